/*
 * r3g.h -- C ABI of libr3g.so: the MI355X-native implementation of the per-object 2D->3D
 * asset-generation hot path of 3D-RE-GEN (stage "Hunyuan_2d_to_3d").
 *
 * The reference has no FFI on this path: its boundary is the Python API of the un-vendored
 * `hy3dgen` package as used by src/2d_to_3d_models/run.py:10-17,77-84 (SURVEY.md section 8b,
 * level B3).  This header is level B4: the plain-C surface that sits directly underneath that
 * Python API.  Each entry point names the reference-side computation it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (R3G_ERR_*); the message of the last
 *    error on the calling thread is available from r3g_last_error();
 *  - pointers named d_* are DEVICE pointers (HBM); h_* are host pointers;
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream); work is enqueued on it and,
 *    unless stated otherwise, the call returns without synchronising;
 *  - no torch / C++ types cross the boundary; one r3g_ctx per process and device, not
 *    thread-safe (mirrors the reference's one-process-per-task model, run.py:108-136);
 *  - there is NO CPU fallback: without a visible gfx950 device r3g_create fails.
 */
#ifndef R3G_H
#define R3G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3G_VERSION 100 /* 0.1.0 */

#define R3G_OK 0
#define R3G_ERR_INVALID (-1)     /* bad argument */
#define R3G_ERR_HIP (-2)         /* HIP runtime error, see r3g_last_error() */
#define R3G_ERR_NO_DEVICE (-3)   /* no gfx950 device visible */
#define R3G_ERR_STATE (-4)       /* call order violated (e.g. emit without count) */
#define R3G_ERR_LEVEL_RANGE (-10) /* skimage: ValueError("Surface level must be within volume data range.") */
#define R3G_ERR_NO_SURFACE (-11)  /* skimage: RuntimeError("No surface found at the given iso value.") */

typedef struct r3g_ctx r3g_ctx;

int r3g_version(void);
const char* r3g_last_error(void);

/* One context per (process, device).  Replaces the implicit CUDA context the reference worker
 * gets from CUDA_VISIBLE_DEVICES (src/2d_to_3d_models/run.py:114). */
int r3g_create(int device, r3g_ctx** out);
void r3g_destroy(r3g_ctx* ctx);

/* ---- marching cubes --------------------------------------------------------------------------
 * Replaces hy3dgen MCSurfaceExtractor.run's
 *     skimage.measure.marching_cubes(grid_logit.cpu().numpy(), mc_level, method="lewiner")
 * (skimage/measure/_marching_cubes_lewiner.py:280-349; reached from run.py:77-84) plus the
 * vertex rescale and winding flip that follow it, with the grid left in HBM.
 *
 * r3g_mc_count: classify all (n0-1)(n1-1)(n2-1) cells of the C-contiguous fp32 grid
 *   d_grid[n0][n1][n2], scan, and report the mesh size.  Synchronises `stream`.
 *   use_classic != 0 selects skimage's method="lorensen" tables.
 *   Errors mirror the wrapper: R3G_ERR_LEVEL_RANGE, R3G_ERR_NO_SURFACE.
 * r3g_mc_emit: write the mesh of the preceding r3g_mc_count (same grid, still resident):
 *   d_verts float32 [nV][3], d_faces int32 [nF][3].
 *   xform == NULL  : skimage's return convention -- vertices in index space, columns
 *                    (axis0, axis1, axis2), faces reversed (gradient_direction='descent').
 *   xform != NULL  : 9 doubles {grid_size[3], bbox_size[3], bbox_min[3]}; vertices become
 *                    float32(double(v) / grid_size * bbox_size + bbox_min) exactly as upstream
 *                    (note upstream's grid_size = R+1), and reverse_faces selects the winding
 *                    (0 = after export_to_trimesh's faces[:, ::-1], i.e. outward for
 *                    positive-inside fields).
 */
int r3g_mc_count(r3g_ctx* ctx, const float* d_grid, int n0, int n1, int n2, double level, int use_classic,
                 int64_t* n_verts, int64_t* n_faces, void* stream);
int r3g_mc_emit(r3g_ctx* ctx, float* d_verts, int32_t* d_faces, const double* xform, int reverse_faces,
                void* stream);

/* ---- dual marching cubes ---------------------------------------------------------------------
 * The extractor behind mc_algo="dmc": one vertex per surface patch of a cell, one quad (two triangles) per crossed
 * grid edge that has four cells around it.  The semantics are this project's own and fixed to the bit in DESIGN.md
 * section 4c; they are not pinned to upstream's extractor.
 *
 * r3g_dmc_count: classify all cells of the C-contiguous fp32 grid d_grid[n0][n1][n2] (inside = value > level), apply
 *   the manifold rule (manifold != 0; 0 is the cross-check form without it), scan, and report the mesh size.
 *   Synchronises `stream`.  R3G_ERR_LEVEL_RANGE under the condition of r3g_mc_count, R3G_ERR_NO_SURFACE when the
 *   mesh has no face.
 * r3g_dmc_emit: write the mesh of the preceding r3g_dmc_count (same grid, still resident): d_verts float32 [nV][3],
 *   d_faces int32 [nF][3].  xform == NULL: index space, columns (axis0, axis1, axis2); otherwise the 9 doubles of
 *   r3g_mc_emit with the same meaning.  reverse_faces == 0: outward for positive-inside fields; != 0: every triangle
 *   (a, b, c) is written (c, b, a).  Without a successful count: R3G_ERR_STATE.
 */
int r3g_dmc_count(r3g_ctx* ctx, const float* d_grid, int n0, int n1, int n2, double level, int manifold,
                  int64_t* n_verts, int64_t* n_faces, void* stream);
int r3g_dmc_emit(r3g_ctx* ctx, float* d_verts, int32_t* d_faces, const double* xform, int reverse_faces,
                 void* stream);

/* ---- mesh cleaners ------------------------------------------------------
 * Replace `mesh = FloaterRemover()(mesh); mesh = DegenerateFaceRemover()(mesh); mesh = FaceReducer()(mesh)`
 * (reference src/2d_to_3d_models/run.py:93-94; upstream hy3dgen/shapegen/postprocessors.py runs pymeshlab on
 * one CPU thread) on the device buffers r3g_mc_emit filled: d_verts float32 [*n_verts][3], d_faces int32
 * [*n_faces][3].  Each call compacts both arrays in place (survivors keep their order), stores the new sizes in
 * *n_verts / *n_faces and synchronises `stream`.
 *   remove_floaters  : drops every connected component with fewer faces than max(1, floor(min_ratio * faces of the largest
 *                      component)) (MeshLab truncates the product), then unreferenced vertices.  Faces are joined through
 *                      shared EDGES, as MeshLab's face-face adjacency joins them: two parts that touch in a single vertex
 *                      are two components (r3g_set_option("floater_by_vertex", 1): joined through shared vertices, the
 *                      behaviour of rounds 1-2).
 *   remove_degenerate: drops faces with a repeated vertex index, then unreferenced vertices.
 *   reduce_faces     : no-op when *n_faces <= max_faces; otherwise quadric-error-metric edge collapse (the algorithm
 *                      class of upstream's MeshLab filter) in rounds of independent collapses: every vertex picks its
 *                      cheapest valid edge (optimal placement; link condition, no face turning by more than ~78
 *                      degrees, no slivers, boundary vertices stay on the boundary) and PROPOSES it; per round a maximal
 *                      set of proposals with pairwise disjoint closed neighbourhoods is selected (three Luby iterations on
 *                      the fixed (key, proposer) order, round 4) and collapses simultaneously, the last round is cut at the key that
 *                      meets the budget (result within 1 % below max_faces).  Closed surfaces stay closed manifolds
 *                      of the same genus.  Equivalence with MeshLab is geometric, not index-wise.
 *   cluster_faces    : vertex clustering on a uniform grid over the bounding box (first resolution
 *                      floor(sqrt(max_faces / 2.2)), shrunk by 0.9 until the face budget holds, at most 24 times): a
 *                      cluster's vertex is the mean of its members, faces that collapse or repeat an earlier face's
 *                      vertex set are dropped.  Robust on triangle soups; does not preserve topology.
 * The results are pure functions of the input: oracle/mesh_clean.py reproduces floaters / degenerate / cluster bit for
 * bit, tests/emu/qem_emu.cpp (the same per-element code in host loops) the edge collapse. */
int r3g_mesh_remove_floaters(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                             double min_ratio, void* stream);
int r3g_mesh_remove_degenerate(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                               void* stream);
int r3g_mesh_reduce_faces(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                          int64_t max_faces, void* stream);
int r3g_mesh_cluster_faces(r3g_ctx* ctx, float* d_verts, int64_t* n_verts, int32_t* d_faces, int64_t* n_faces,
                           int64_t max_faces, void* stream);

/* ---- mesh distance -----------------------------------------------------------------
 * Exact nearest-triangle query, the primitive under Chamfer / Hausdorff / F-score (r3g/meshdist.py): how far two meshes
 * lie apart in space, e.g. the exact extraction against one of the opt-in approximations.
 *
 * r3g_meshdist_build: take the target mesh (d_verts float32 [n_verts][3], d_faces int32 [n_faces][3]) into a uniform grid over
 *   its bounding box, in CSR form, built on the device (count, scan, fill).  resolution = cells per axis, 1..256; 0 = automatic:
 *   floor(sqrt(n_faces / 2)) capped at 256, halved while the grid holds more than 8 * n_faces (face, cell) pairs.  Resolution 1
 *   is brute force.  *resolution_out = the resolution used, *pairs_out = the pairs stored, *skipped_out = faces with a
 *   non-finite vertex (they take part in nothing); each may be NULL.  The build copies what the query needs: the mesh buffers
 *   may be freed afterwards.  Synchronises `stream`.  Errors: a face index outside [0, n_verts) is found on the device before
 *   anything is read through it and fails the call with -2; n_faces == 0 or a mesh whose every face is skipped:
 *   R3G_ERR_INVALID.  A failed build leaves the context without a grid.
 * r3g_meshdist_query: for each of d_points float32 [n_points][3]
 *       d_dist2[i] = min over the usable faces t of tri_dist2(p_i, t)      (csrc/meshdist_core.h: one float32 function)
 *       d_face[i]  = the lowest face index attaining it
 *   against the grid of the last successful build on this context (none: R3G_ERR_STATE).  A point with a non-finite coordinate
 *   gets NaN and -1.  The result is a pure function of the mesh and the points: it depends neither on the resolution nor on
 *   the order in which the build's integer atomics land (tests/emu/meshdist_emu.cpp reproduces it bit for bit on the host).
 *   n_points == 0 is a no-op.  Synchronises `stream` (the number of point-triangle tests is read back into the counter
 *   "meshdist_tests"). */
int r3g_meshdist_build(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces,
                       int resolution, int* resolution_out, int64_t* pairs_out, int64_t* skipped_out, void* stream);
int r3g_meshdist_query(r3g_ctx* ctx, const float* d_points, int64_t n_points, float* d_dist2, int32_t* d_face, void* stream);

/* ---- point in mesh -------------------------------------------------------------------
 * Ray-crossing count, the primitive under contains / signed distance / volumetric IoU (r3g/meshinside.py): on which side of
 * a surface a point lies, which the unsigned distance above cannot tell.
 *
 * r3g_meshinside_build: take the mesh (d_verts float32 [n_verts][3], d_faces int32 [n_faces][3]) into a grid of R x R columns
 *   over its bounding box projected along `axis` (0, 1, 2 = x, y, z: the direction of the rays), in CSR form, built on the
 *   device (count, scan, fill).  resolution = columns per projected axis, 1..1024; 0 = automatic: floor(sqrt(n_faces)) capped
 *   at 1024, halved while the grid holds more than 8 * n_faces (face, column) pairs.  Resolution 1 is brute force.
 *   *resolution_out = the resolution used, *pairs_out = the pairs stored, *skipped_out = faces with a non-finite vertex (they
 *   take part in nothing); each may be NULL.  Faces whose projection has zero area take part in nothing either and are not
 *   counted as skipped.  The build copies what the query needs: the mesh buffers may be freed afterwards.  The grid is
 *   separate from the one of r3g_meshdist_build: a context holds both at once.  Synchronises `stream`.  Errors: a face index
 *   outside [0, n_verts) is found on the device before anything is read through it and fails the call with -2; axis outside
 *   0..2, a resolution outside [0, 1024], n_faces == 0 or a mesh whose every face is skipped: R3G_ERR_INVALID.  A failed build
 *   leaves the context without a grid.
 * r3g_meshinside_query: for each of d_points float32 [n_points][3]
 *       d_count[i] = the number of usable faces t with crossed(p_i, t)      (csrc/meshinside_core.h: float64 arithmetic on
 *                    the float32 inputs, one operation per difference and product)
 *   i.e. the faces the ray from p_i in the +axis direction crosses, against the grid of the last successful build on this
 *   context (none: R3G_ERR_STATE).  p_i is inside when the count is odd.  A ray through a shared edge or vertex is decided by
 *   one rule for both faces (E == 0 counts as the positive side of the edge's canonical direction), so a closed surface is
 *   crossed once where it continues and twice or not at all where it folds back; a point exactly on a face is not below it.
 *   A point with a non-finite coordinate gets -1.  The result is a pure function of the mesh, the axis and the points: it
 *   depends neither on the resolution nor on the order in which the build's integer atomics land
 *   (tests/emu/meshinside_emu.cpp reproduces it exactly on the host).  n_points == 0 is a no-op.  Synchronises `stream` (the
 *   number of point-face tests is read back into the counter "meshinside_tests"). */
int r3g_meshinside_build(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces,
                         int axis, int resolution, int* resolution_out, int64_t* pairs_out, int64_t* skipped_out, void* stream);
int r3g_meshinside_query(r3g_ctx* ctx, const float* d_points, int64_t n_points, int32_t* d_count, void* stream);

/* ---- mesh registration ----------------------------------------------------------------
 * Closest points and iterative closest point (ICP) of a point set onto a mesh, the alignment that the distances above
 * presuppose (r3g/meshfit.py).  All three calls work against the grid of the last successful r3g_meshdist_build on the
 * context (none: R3G_ERR_STATE) and leave it as it is.
 *
 * r3g_meshdist_closest: r3g_meshdist_query plus the point that attains the distance: d_closest float32 [n_points][3] =
 *   tri_closest(p_i, face) (csrc/meshdist_core.h: candidates in the order edge ab, bc, ac, interior; a later one wins only
 *   when strictly nearer), d_dist2 and d_face exactly as r3g_meshdist_query gives them.  A point with a non-finite coordinate
 *   gets NaN, -1 and NaN.  n_points == 0 is a no-op.  Enqueues on `stream` and does not synchronise.
 * r3g_meshfit_step: ONE accumulation of the registration, no solve.  xform = 13 doubles: s, R (row-major, 9), t.  Each source
 *   point d_points[i] (float32) is moved to p' = s R p + t in float64 and rounded to float32; q = the closest point of the mesh
 *   to p', d2 its squared distance.  The point takes part iff p' is finite and d2 <= (float)(max_dist^2) (max_dist = +inf: every
 *   finite point), with weight w_i = d_weights[i] (float32, finite, >= 0; NULL: 1).  mode 0 (point): sums_out[0..18) =
 *   W, sum w p', sum w q, sum w p' q^T (row = p'), sum w |p'|^2, sum w d2.  mode 1 (plane): sums_out[0..37) = the upper triangle
 *   of sum w j j^T (28, row-major), sum w j r (7), W, sum w d2, with j = [p' x n, n, p' . n], r = n . (q - p'), n the unit normal
 *   of the winning face ((p' - q) / |p' - q| for a face without area; a point with neither adds W and d2 only), evaluated
 *   without a square root as (w / N.N) J J^T and (w / N.N) J R on the unnormalised normal N.  p' and q are taken relative to
 *   the centre of the grid's box, c = (lo + hi) / 2 in float64.  sums_out must hold 37 doubles (host memory); *used_out = the points
 *   that took part.  The sums are added in float64 in a fixed order (wave butterfly, the block's four waves in
 *   index order, the blocks' records in index order by the same tree; no floating-point atomics), so they are a pure function
 *   of the mesh, the points, the weights and xform, independent of the grid's resolution; tests/emu/meshfit_emu.cpp reproduces
 *   them bit for bit on the host.  n_points == 0 gives zeros.  Synchronises `stream`.
 * r3g_meshfit: the loop accumulate -> solve -> compose on the host.  init = row-major 4 x 4 similarity (NULL: identity; not
 *   a similarity with positive determinant: R3G_ERR_INVALID).  mode 1 = point-to-plane (one Gauss-Newton step per iteration:
 *   Cholesky of the 6 x 6 normal equations, 7 x 7 with_scale; an unconstrained degree of freedom stays 0), mode 0 = the closed
 *   form on closest points (Horn / Umeyama).  Each iteration accumulates under the current transform and stops, before solving,
 *   when |rms_prev - rms| < tolerance or when max_iterations updates have been made; so matrix_out (row-major 4 x 4, maps
 *   source onto target) is the transform the last accumulation ran under.  info_out = 5 doubles: updates made, converged (0 | 1),
 *   rms = sqrt(sum w d2 / W) of the last accumulation, points used in it, scale of matrix_out.  Errors: mode outside 0..1,
 *   max_dist < 0 or NaN, max_iterations < 0, tolerance NaN: R3G_ERR_INVALID; an accumulation with fewer than 3 points used or
 *   W <= 0: R3G_ERR_INVALID ("too few points"), matrix_out untouched.  n_points == 0: matrix_out = init, used 0, rms 0.
 *   Synchronises `stream` once per accumulation (one 320-byte read-back through a pinned buffer of the context). */
int r3g_meshdist_closest(r3g_ctx* ctx, const float* d_points, int64_t n_points, float* d_dist2, int32_t* d_face, float* d_closest,
                         void* stream);
int r3g_meshfit_step(r3g_ctx* ctx, const float* d_points, int64_t n_points, const float* d_weights, const double* xform, int mode,
                     double max_dist, double* sums_out, int64_t* used_out, void* stream);
int r3g_meshfit(r3g_ctx* ctx, const float* d_points, int64_t n_points, const float* d_weights, const double* init, int mode,
                int with_scale, int max_iterations, double tolerance, double max_dist, double* matrix_out, double* info_out,
                void* stream);

/* ---- mesh topology --------------------------------------------------------------------
 * Is the mesh a valid surface -- closed, manifold, consistently wound -- and the in-place repair of its winding
 * (r3g/meshtopo.py; trimesh's face_adjacency, is_watertight, is_winding_consistent, euler_number, volume, area,
 * repair.fix_winding, repair.fix_normals, repair.broken_faces).  Everything is a pure function of d_faces and n_verts, and
 * for volume and area of d_verts (csrc/meshtopo_core.h; tests/emu/meshtopo_emu.cpp reproduces it exactly on the host): integer
 * atomics only, and the order in which they land decides nothing.
 *
 * r3g_meshtopo_build: take the mesh (d_verts float32 [n_verts][3] or NULL, d_faces int32 [n_faces][3]) and leave on the context
 *   mate int32 [n_faces][3], body int32 [n_faces], flip uint8 [n_faces] and the report.  A face is USABLE when its three indices are
 *   pairwise different; the others are counted in `skipped` and take part in nothing.  Half-edge h = 3 f + k of usable face f runs
 *   from v_k to v_(k+1)%3; an undirected edge has deg half-edges, n_fwd of them running from its lower to its higher vertex.
 *       mate[h] = the other half-edge (deg = 2) | -1 boundary (deg = 1) | -2 non-manifold (deg >= 3) | -3 skipped face
 *   A deg = 2 edge whose two half-edges run in the same direction is a CLASH.  Faces joined through deg = 2 edges form a body;
 *   body[f] = the lowest face index of the body (-1: skipped).  A body is orientable iff bits flip[f] exist with
 *   flip[f] ^ flip[g] = (the edge between f and g is a clash) over all its deg = 2 edges; flip is the one such assignment with
 *   flip[body[f]] = 0, and 0 on every face of an unorientable body.
 *   report (int64 [16], may be NULL): 0 usable faces, 1 skipped, 2 referenced vertices, 3 distinct edges, 4 boundary edges,
 *   5 clashes, 6 non-manifold edges, 7 bodies, 8 unorientable bodies, 9 euler = [2] - [3] + [0], 10 nonfinite (usable faces with
 *   a non-finite vertex), 11 six_volume_q, 12 its scale exponent s_vol, 13 two_area_q, 14 its scale exponent s_area, 15 whether
 *   d_verts was given ([10] - [14] are 0 without).  six_volume_q = sum of llrint(det[a, b, c] * 2^s_vol) and two_area_q = sum of
 *   llrint(|ab x ac| * 2^s_area) over the usable faces without a non-finite vertex (float64 arithmetic on the float32 inputs);
 *   with e such that the largest finite |coordinate| of a referenced vertex is below 2^e, s_vol = 30 - 3 e and s_area = 29 - 2 e,
 *   so 2^29 faces cannot overflow and |sum / 2^s - exact sum| <= faces * 2^-(s + 1).  watertight = ([0] > 0 and [4] == 0 and
 *   [6] == 0); winding consistent = ([5] == 0).
 *   A face index outside [0, n_verts): error -2, found on the device before anything is read through the index.  n_faces == 0 or
 *   above 2^29: R3G_ERR_INVALID.  The body labels are found in rounds (counter "meshtopo_rounds") until one changes nothing; 1024
 *   rounds without that: R3G_ERR_INVALID, and no partial labelling is kept.  A failed build leaves the context without a state.
 *   Synchronises `stream` (one 136-byte read-back per round through a pinned buffer of the context).
 * r3g_meshtopo_report / _mates / _bodies: the report, mate (d_mate int32 [n_faces][3]) and body / flip (either may be NULL) of the
 *   last successful build or orient on this context (none: R3G_ERR_STATE).  The copies are enqueued on `stream`.
 * r3g_meshtopo_orient: build, then rewrite d_faces in place -- a reversed face (v0, v1, v2) becomes (v2, v1, v0) -- so that every
 *   orientable body is consistently wound (the faces with flip = 1 are reversed), and with outward = 1 (trimesh's multibody = True)
 *   every orientable body whose quantised volume is then negative is reversed as a whole, with outward = 2 (trimesh's default)
 *   every orientable body if the sum of the orientable bodies' volumes is then negative (the unorientable bodies, which are
 *   never reversed, are left out of that sum: reversing what may be reversed negates it exactly, so the result is stable).
 *   outward = 0 looks at no volume; 1 and 2 need d_verts.  A zero sum
 *   changes nothing, unorientable bodies are never touched, and a face that both steps would reverse is not written at all.
 *   *faces_reversed = the faces rewritten, *bodies_reversed = the bodies the outward step reversed (either may be NULL).  The state
 *   left on the context describes the faces as this call leaves them (a second build when anything was reversed); a second call on
 *   its own output reverses nothing.  Errors as r3g_meshtopo_build; outward outside 0..2: R3G_ERR_INVALID. */
int r3g_meshtopo_build(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces, int64_t* report,
                       void* stream);
int r3g_meshtopo_report(r3g_ctx* ctx, int64_t* report);
int r3g_meshtopo_mates(r3g_ctx* ctx, int32_t* d_mate, void* stream);
int r3g_meshtopo_bodies(r3g_ctx* ctx, int32_t* d_body, uint8_t* d_flip, void* stream);
int r3g_meshtopo_orient(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, int32_t* d_faces, int64_t n_faces, int outward,
                        int64_t* faces_reversed, int64_t* bodies_reversed, void* stream);

/* ---- mesh fill ------------------------------------------------------------------------
 * Close the holes of a triangle mesh: chain the boundary half-edges of the mate table of section 4i into loops and append the
 * faces that close each loop (r3g/meshfill.py; trimesh's repair.fill_holes).  Everything is a pure function of d_faces, n_verts,
 * max_loop and mode, and for the centroids of d_verts (csrc/meshfill_core.h; tests/emu/meshfill_emu.cpp reproduces it exactly on
 * the host): integer atomics only, and the order in which they land decides nothing.
 *
 * A half-edge h is a BOUNDARY half-edge iff mate[h] = -1.  nout[v] / nin[v] count the boundary half-edges with tail / head v; v is
 * SIMPLE iff nout[v] = nin[v] = 1.  succ[h] = the boundary half-edge whose tail is head(h) if head(h) is simple, else -1.  A LOOP is
 * a cycle of succ; a boundary half-edge on no cycle is TANGLED (pinch vertices, chains through inconsistently wound faces, edges
 * beside a non-manifold vertex) and is never filled.  A loop's LEADER is its lowest half-edge id, rank[h] the succ steps from the
 * leader to h, L its length (L >= 3), its vertices a_i = tail of the half-edge of rank i.  A loop with L > max_loop is OVERSIZE and
 * left alone.  The filled loops are numbered j = 0, 1, ... by ascending leader; the faces of loop j follow those of loop j - 1:
 *     mode 0 (fan, no new vertex):         (a_0, a_(i+1), a_i)       for i = 1 .. L - 2
 *     mode 1 (centroid, one new vertex):   (c_j, a_(i+1)%L, a_i)     for i = 0 .. L - 1,  c_j = n_verts + j
 *   The centroid is, per coordinate, the float64 sum of the float32 values in rank order (one rounding per addition), the float64
 *   quotient by L, converted once to float32; non-finite inputs propagate.  Every new face carries the reverse of each boundary
 *   half-edge it closes, so it is wound like its neighbours.  A fan diagonal may repeat an edge the mesh has elsewhere; that edge
 *   is then non-manifold in the result (it shows in the result's topology report; it is not prevented).
 *
 * r3g_meshfill_plan: run r3g_meshtopo_build on the mesh (its state stays on the context and describes the input mesh), find the
 *   loops and leave on the context what _emit and _loops need.  d_verts may be NULL in mode 0.
 *   report (int64 [16], may be NULL): 0 boundary half-edges, 1 loops, 2 tangled half-edges, 3 filled loops, 4 oversize loops,
 *   5 longest loop, 6 loop_edges (sum of L over all loops; [2] = [0] - [6]), 7 faces_added, 8 verts_added, 9 rounds (of each of the
 *   two pointer doublings: ceil(log2 max([0], 2)), 0 without a boundary), 10 max_loop, 11 mode, 12 n_faces, 13 n_verts, rest 0.
 *   n_faces == 0 or above 2^29, max_loop < 3, a mode other than 0 or 1, mode 1 without d_verts, or n_verts + verts_added beyond
 *   int32: R3G_ERR_INVALID; a face index outside [0, n_verts): -2, as r3g_meshtopo_build.  A failed plan leaves the context
 *   without a fill state.  Synchronises `stream` (the read-backs of the topology build and one 40-byte read-back of its own).
 * r3g_meshfill_emit: write the appended elements only -- d_new_faces int32 [faces_added][3] and, in mode 1, d_new_verts float32
 *   [verts_added][3] (may be NULL: not written); the caller concatenates.  Nothing to add: nothing is written, buffers may be NULL.
 * r3g_meshfill_loops: every loop, filled or not, ascending by leader, each in rank order: d_loop_start int64 [loops + 1],
 *   d_loop_verts int32 [loop_edges], d_loop_status int32 [loops] (0 filled, 1 oversize; the last two may be NULL without a loop).
 * _emit and _loops without a successful plan on this context: R3G_ERR_STATE.  Both are enqueued on `stream`. */
int r3g_meshfill_plan(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_faces, int64_t n_faces, int64_t max_loop,
                      int mode, int64_t* report, void* stream);
int r3g_meshfill_emit(r3g_ctx* ctx, int32_t* d_new_faces, float* d_new_verts, void* stream);
int r3g_meshfill_loops(r3g_ctx* ctx, int64_t* d_loop_start, int32_t* d_loop_verts, int32_t* d_loop_status, void* stream);

/* ---- point clouds: exact k nearest neighbours ---------------------------------------------------
 * Point against point, where sections 4f-4h are point against triangle (r3g/cloud.py builds the reference's evaluation scores,
 * normals and cloud ICP on it).  For a query p and a target point q_i, d2(p, q_i) = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2 in
 * float32, one rounding per operation, left to right, no contraction (csrc/cloud_core.h; tests/emu/cloud_emu.cpp reproduces it
 * exactly on the host).  The answer for k is the k smallest pairs (d2, i) in lexicographic order, ascending; equal coordinates
 * under distinct indices are distinct neighbours.  The grid only prunes: the result does not depend on the resolution.
 *
 * r3g_cloud_build: take the target points (d_points float32 [n_points][3]) into a uniform grid of resolution^3 cells over their
 *   bounding box; resolution 0 = automatic, min(256, max(1, floor(cbrt(usable / P)))) with P = 1 point per cell.  A point with a non-finite coordinate is
 *   left out and counted in *skipped_out; indices stay those of d_points.  The context keeps a packed copy of its own in cell order
 *   (16 bytes a point), so d_points may be freed afterwards; the copy is separate from the grids of r3g_meshdist_build and
 *   r3g_meshinside_build, a context holds all three at once.  Synchronises `stream`.  n_points == 0 or above 2^31 - 1, no usable
 *   point, a resolution outside [0, 256]: R3G_ERR_INVALID, before any launch where the sizes show it.  A failed build leaves the
 *   context without a cloud.  The out pointers may be NULL.
 * r3g_cloud_knn: for each of d_queries float32 [n_queries][3] its k nearest target points, k in [1, 32] (else R3G_ERR_INVALID):
 *   d_dist2 float32 [n_queries][k] and d_index int32 [n_queries][k], ascending by (d2, index).  With fewer than k usable points
 *   the remaining slots are (+inf, -1); a query with a non-finite coordinate gets (NaN 0x7fc00000, -1) in every slot.  Without a
 *   successful build on this context: R3G_ERR_STATE.  n_queries == 0: success, nothing launched.  Synchronises `stream` (one
 *   read-back: counter "cloud_tests"). */
int r3g_cloud_build(r3g_ctx* ctx, const float* d_points, int64_t n_points, int resolution, int* resolution_out, int64_t* skipped_out,
                    void* stream);
int r3g_cloud_knn(r3g_ctx* ctx, const float* d_queries, int64_t n_queries, int k, float* d_dist2, int32_t* d_index, void* stream);

/* ---- point clouds: consistent orientation of normals --------------------------------------------
 * The sign of every normal by propagation over the minimum spanning forest of the k-nearest-neighbour graph (Hoppe).  A point is
 * usable when its coordinates and normal are finite and the normal is non-zero.  {i, j} is an edge when j is among the k nearest
 * usable neighbours of i other than i, or the other way round (the (k + 1)-list of r3g_cloud_knn of the usable points against
 * themselves, without the entry i, or without the last one when i is absent).  w(i, j) = 1 - |u_i . u_j| in float32 on the unit
 * normals; edges are totally ordered by (w, min(i, j), max(i, j)), so the forest is unique.  Along every forest edge
 * s_i s_j = (u_i . u_j >= 0 ? +1 : -1); in every tree the member with the largest z (the lowest index on a tie) ends with
 * s n_z >= 0 (+1 where n_z == 0).  csrc/orient_core.h; tests/emu/orient_emu.cpp reproduces it exactly on the host.
 *
 * r3g_cloud_orient: d_points, d_normals float32 [n_points][3], k in [1, 31] -> d_sign int8 [n_points] (+1 keep, -1 reverse, 0 for
 *   a point that is not usable) and d_tree int32 [n_points] (the lowest index of the point's tree, -1 for a point that is not
 *   usable).  report (int64 [8], may be NULL): usable points, trees, signs that are -1, Boruvka rounds launched (the last one
 *   merges nothing), frustrated graph edges (their ends disagree with s_i s_j above: a quality figure, not an error), 0, 0, 0.
 *   The call REPLACES the cloud of r3g_cloud_build on this context by the usable points, built at `resolution` (0 = automatic; the
 *   grid only prunes, the result does not depend on it).  n_points == 0 or above 2^31 - 1, k outside [1, 31], a resolution outside
 *   [0, 256], a null buffer: R3G_ERR_INVALID before any launch.  No usable point: success, every sign 0.  Synchronises
 *   `stream` (one small read-back per round: counter "orient_rounds"). */
int r3g_cloud_orient(r3g_ctx* ctx, const float* d_points, const float* d_normals, int64_t n_points, int k, int resolution, int8_t* d_sign,
                     int32_t* d_tree, int64_t* report, void* stream);

/* ---- point clouds: DBSCAN ---------------------------------------------------------------------
 * The clustering that the reference's filter_dbscan asks of scikit-learn, with scikit-learn's labels.  A point is usable when its
 * three coordinates are finite; an unusable point is nobody's neighbour.  q is a neighbour of p iff d2 = ((dx*dx) + dy*dy) + dz*dz
 * <= eps*eps with every coordinate widened to float64 first, one rounding per operation, left to right, no contraction, eps*eps
 * computed once in float64 (csrc/dbscan_core.h; tests/emu/dbscan_emu.cpp reproduces it exactly on the host).  A point is its own
 * neighbour; equal coordinates under distinct indices are distinct neighbours.  count[i] = the neighbours of i, itself included;
 * i is a core point iff count[i] >= min_samples.  Clusters are the connected components of the core points under the neighbour
 * relation, numbered 0, 1, ... in ascending order of their smallest core index.  label[i]: a core point's cluster; for a
 * non-core point with a core neighbour (a border point) the smallest cluster number among its core neighbours; otherwise -1.
 *
 * r3g_cloud_dbscan: d_points float32 [n_points][3] -> d_label int32 [n_points] and, where d_count is not NULL, d_count uint32
 *   [n_points] (0 for an unusable point; without d_count a point stops counting at min_samples, which changes no label).
 *   report (int64 [8], may be NULL): usable points, core points, border points, noise points (usable, label -1), clusters, the
 *   largest cluster (most points, the lowest number on a tie, -1 without a cluster), its size, the resolution used.
 *   The call REPLACES the cloud of r3g_cloud_build on this context by the usable points (r3g_cloud_knn may follow it), built at
 *   `resolution` cells per axis; 0 = automatic: floor(longest box extent / eps), at least 1, at most 256 and at most the largest
 *   r with r^3 <= 8 * usable.  The grid only prunes, the result does not depend on it.  The number of kernel launches does not
 *   depend on the data (counter "dbscan_launches"; "dbscan_tests" counts the evaluations of the neighbour predicate).
 *   eps not finite or <= 0, min_samples < 1, n_points < 0 or above 2^31 - 1, a resolution outside [0, 256], a null buffer with
 *   n_points > 0: R3G_ERR_INVALID before any launch.  n_points == 0 and a cloud without a usable point succeed, every label -1
 *   and the report zero but for largest = -1; they leave the context without a cloud.  Synchronises `stream`.
 * r3g_cloud_dbscan_times: milliseconds of the last complete r3g_cloud_dbscan on this context between HIP events on its stream,
 *   ms double [5]: grid build, count pass, link pass (with its flatten), border pass, numbering (with sizes and the largest
 *   cluster).  Without such a call: R3G_ERR_STATE. */
int r3g_cloud_dbscan(r3g_ctx* ctx, const float* d_points, int64_t n_points, double eps, int min_samples, int resolution, int32_t* d_label,
                     uint32_t* d_count, int64_t* report, void* stream);
int r3g_cloud_dbscan_times(r3g_ctx* ctx, double* ms);

/* ---- point clouds: plane fit ---------------------------------------------------------------------
 * The initialisation of the reference's pose matching: fit_plane_ransac_refined as one batch of hypotheses, and the moments
 * behind fit_plane_svd and the PCA test of extract_and_fit_floor_plane.  A point is usable when its three coordinates are finite.
 * Hypothesis h is a triple of row indices (i0, i1, i2); with every coordinate widened to float64, one rounding per operation, no
 * contraction: v1 = p[i1] - p[i0], v2 = p[i2] - p[i0], c = v1 x v2, len = sqrt((cx*cx + cy*cy) + cz*cz).  It is valid when the
 * three indices lie in [0, n_points), the three points are usable and len >= 1e-6; its unit normal is c / len.  q is an inlier
 * of h iff |((qx-p0x)*nx + (qy-p0y)*ny) + (qz-p0z)*nz| < threshold in float64; an unusable point is never an inlier.  count[h] =
 * the inliers of h, 0 for an invalid hypothesis.  The winner is the valid hypothesis with the largest count, the lowest h on a
 * tie.  The moments of a set of rows are n, sum p, the centroid sum p / n and the scatter sum (p - c)(p - c)^T, float64 sums in
 * the one fixed order written in csrc/plane_core.h (it depends on n_points alone); the eigenpairs of the scatter come from the
 * cyclic Jacobi of that header, run on the host.  The normal of a set is the eigenvector of its smallest eigenvalue, turned so
 * that n_y >= 0; a set of fewer than 3 rows gets (0, 1, 0), zero eigenvalues and a flag.  tests/emu/plane_emu.cpp reproduces
 * every bit on the host.
 *
 * r3g_plane_ransac: d_points float32 [n_points][3], d_triples int32 [n_hyp][3] -> where not NULL, d_count uint32 [n_hyp] and d_mask
 *   uint8 [n_points] (1 for the winner's inliers, all 0 without a winner).  report (int64 [8]): usable points, valid hypotheses,
 *   the winner h (-1 without one), its count, 1 when the refinement saw fewer than 3 rows, 0, 0, 0.  plane (double [16], host): the
 *   winner's p0 [0..2] and unit normal [3..5] (zeros without one), the inliers' centroid [6..8], the refined normal [9..11], the
 *   eigenvalues of their scatter ascending [12..14], 0.  The number of kernel launches does not depend on the data: the table,
 *   the count pass (every point is tested against every valid hypothesis; counts by ballot, combined with integer atomics), the
 *   arg-max, the mask and four for the moments.  threshold not finite or <= 0, n_hyp < 0 or above 65536, n_points < 0 or above
 *   2^31 - 1, report or plane NULL, d_points NULL with n_points > 0, d_triples NULL with n_hyp > 0: R3G_ERR_INVALID before any
 *   launch.  n_points == 0, n_hyp == 0 and a table without a valid entry succeed with winner -1.  Synchronises `stream` once.
 * r3g_plane_moments: the rows of d_points with d_mask[i] != 0 (every row when d_mask is NULL) -> out (double [16], host): n, the
 *   centroid [1..3], the scatter xx, xy, xz, yy, yz, zz [4..9], the eigenvalues ascending [10..12], the normal [13..15].  report
 *   (int64 [4]): rows in the set, selected rows left out as unusable, 1 for fewer than 3 rows, 0.  n_points < 0 or above 2^31 - 1,
 *   out or report NULL, d_points NULL with n_points > 0: R3G_ERR_INVALID before any launch.  Synchronises `stream` once.
 * r3g_plane_times: milliseconds of the last complete r3g_plane_ransac on this context between HIP events on its stream, ms double
 *   [4]: table, count pass, winner and mask, moments.  Without such a call: R3G_ERR_STATE. */
int r3g_plane_ransac(r3g_ctx* ctx, const float* d_points, int64_t n_points, const int32_t* d_triples, int n_hyp, double threshold,
                     uint32_t* d_count, uint8_t* d_mask, int64_t* report, double* plane, void* stream);
int r3g_plane_moments(r3g_ctx* ctx, const float* d_points, int64_t n_points, const uint8_t* d_mask, double* out, int64_t* report,
                      void* stream);
int r3g_plane_times(r3g_ctx* ctx, double* ms);

/* ---- soft silhouettes: differentiable K-nearest rasteriser ------------------------------------------
 * The renderer of the reference's planar pose fit (pytorch3d's MeshRasterizer with a blur radius and SoftSilhouetteShader), and
 * its gradient to the vertices.  d_pos float32 [n_verts][3] = (x, y, z): x, y in pixels, pixel (row i, column j) samples the
 * point (j + 0.5, i + 0.5), row 0 is the top; z is the view depth.  d_tri int32 [n_faces][3].  All arithmetic is float32, one
 * rounding per operation, no contraction; the definition is the text of csrc/softras_core.h and tests/emu/softras_emu.cpp
 * reproduces every bit on the host.
 *   A face is skipped when an index lies outside [0, n_verts), when one of its nine coordinates is NaN, infinite or larger than
 *   1e15 in magnitude, when its edge function |area| <= 1e-8, or when its three z are < 0.  At pixel centre p a face has the
 *   barycentrics b_i = edge_i(p) / area; clipped, c_i = max(b_i, 0) / max(sum, 1e-5); pz = (c0 z0 + c1 z1) + c2 z2; inside = all
 *   b_i > 0; d2 = the smallest squared distance from p to the three segments (v0 v1), (v1 v2), (v2 v0), the first on a tie, with
 *   t = dot(v1 - v0, p - v0) / |v1 - v0|^2 clamped to [0, 1] and an edge with |v1 - v0|^2 <= 1e-8 measured to v1; dist = inside ?
 *   -d2 : d2.  The fragment is kept when (inside or d2 < blur_radius) and not pz < 0.  A pixel keeps the K fragments with the
 *   smallest key (pz, face index), in ascending order.  alpha = 1 - prod_k (1 - s_k) in list order, s_k = sr_sigmoid(-dist_k /
 *   sigma), sr_sigmoid(x) = 1 / (1 + sr_exp(-clamp(x, -80, 80))).
 * r3g_softras_forward: -> d_alpha float32 [height][width], d_face int32 [height][width][K] (-1: empty slot), d_dist and d_zbuf
 *   float32 [height][width][K] (-1 in an empty slot).  report (int64 [8]): (face, 8 x 8 tile) pairs of the bin pass, faces drawn
 *   whose box meets the image, faces skipped, tiles, 0, 0, 0, 0.  Launches: count, the scan's three, fill, forward.  Synchronises
 *   `stream` once, after the count (the pair list is sized from it); the forward kernel is queued behind it.  n_faces == 0
 *   gives alpha 0 and face -1 everywhere.  More than 2^31 - 1 pairs: R3G_ERR_INVALID.
 * r3g_softras_backward: d_face, d_dist as the forward wrote them for the same mesh and arguments, d_grad_alpha float32
 *   [height][width] -> d_grad_face float32 [n_faces][3][2] (the gradient to the xy of each face's corners) and d_grad_pos float32
 *   [n_verts][3] (z column 0).  d alpha / d dist_k = -(s_k (1 - s_k) prod_{j != k} (1 - s_j)) / sigma, the exclusive product
 *   multiplied out in list order; d dist / d xy follows the forward's branch (the winning edge, t clamped or not, the sign of
 *   inside).  A pixel whose grad_alpha is NaN or infinite contributes nothing.  One workgroup per face sums in the fixed order of
 *   csrc/softras_core.h; a vertex sums its corners d_corner_ids[d_corner_start[v] .. d_corner_start[v + 1]) (int32; corner 3 f +
 *   a, ascending) sequentially: no floating-point atomics, the same bits on every call.  report (int64 [4]): (pixel, face)
 *   fragments found in the stored lists, 0, 0, 0.  Synchronises `stream` once.
 * Both: K outside 1 .. 32, sigma not finite or <= 0 (as float32), blur_radius negative or NaN, height or width outside
 *   [1, 16384], n_verts or n_faces negative, n_faces above 2^29, a NULL buffer with a non-zero size, report NULL: R3G_ERR_INVALID
 *   before any launch.
 * r3g_softras_times: milliseconds between HIP events of the last complete calls on this context, ms double [4]: bin (with its
 *   read-back), forward, backward, gather; -1 for the last two while no backward has run.  Waits for the forward's kernel.
 *   Without a forward: R3G_ERR_STATE. */
int r3g_softras_forward(r3g_ctx* ctx, const float* d_pos, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, int height, int width,
                        int K, double sigma, double blur_radius, float* d_alpha, int32_t* d_face, float* d_dist, float* d_zbuf,
                        int64_t* report, void* stream);
int r3g_softras_backward(r3g_ctx* ctx, const float* d_pos, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, int height, int width,
                         int K, double sigma, double blur_radius, const int32_t* d_face, const float* d_dist, const float* d_grad_alpha,
                         const int32_t* d_corner_start, const int32_t* d_corner_ids, float* d_grad_face, float* d_grad_pos,
                         int64_t* report, void* stream);
int r3g_softras_times(r3g_ctx* ctx, double* ms);

/* ---- point clouds: every triangle's nearest point ---------------------------------------------------
 * The face -> point half of pytorch3d's point_mesh_face_distance, against the cloud on this context (the last successful
 * r3g_cloud_build, r3g_cloud_orient or r3g_cloud_dbscan), which the calls read and leave as it is.  For a triangle t and the
 * usable points p_i: d2(t) = min_i tri_dist2(p_i, t), section 4f's float32 function without contraction, index(t) = the lowest
 * original index attaining it: the minimum of (d2, i) in lexicographic order.  Beside it come r, the closest point of t to
 * p_index, as barycentric weights w[3] (r = w0 a + w1 b + w2 c up to rounding; the s, v, w that formed r), and diff = p_index - r.
 * A triangle without area is served by its edges; there is no min_triangle_area.  The definition is the text of
 * csrc/facecloud_core.h and tests/emu/facecloud_twin.cpp reproduces every bit on the host.  The grid only prunes: the result does
 * not depend on the cloud's resolution.
 *
 * r3g_cloud_faces: d_verts float32 [n_verts][3], d_tri int32 [n_faces][3] -> d_dist2 float32 [n_faces], d_index int32 [n_faces],
 *   d_weights float32 [n_faces][3], d_diff float32 [n_faces][3].  A face is unusable when an index lies outside [0, n_verts) or a
 *   vertex is not finite: it gets d2 = NaN 0x7fc00000, index -1, weights 0, diff 0, and nothing is read through its indices.
 *   report (int64 [4]): usable faces, point-triangle tests, faces walked by a wave (a cell box of more than 64 cells), the largest
 *   ring walked.  Launches: classify, narrow, wide.  Synchronises `stream` once, for the report.  Without a cloud on this context:
 *   R3G_ERR_STATE.  n_faces == 0: success, a zero report, nothing launched.  n_verts or n_faces negative, n_verts above 2^31 - 1,
 *   n_faces above 2^29, report NULL, d_tri or an output NULL with n_faces > 0, d_verts NULL with n_verts > 0: R3G_ERR_INVALID before
 *   any launch.
 * r3g_cloud_faces_backward: d_grad_dist2 float32 [n_faces], and d_index, d_weights, d_diff as the forward wrote them ->
 *   d_grad_verts float32 [n_verts][3].  With w and index held constant d d2 / d vertex_a = -2 w_a diff, which is the exact
 *   gradient wherever the distance is differentiable.  A vertex sums its corners d_corner_ids[d_corner_start[v] ..
 *   d_corner_start[v + 1]) (int32; corner 3 f + a, ascending: section 4o's lists) sequentially in float32, each corner adding
 *   g_f * (-2 w[f][a]) * diff[f]: no floating-point atomics, the same bits on every call.  A corner adds nothing when its face is
 *   unusable or its g_f is NaN or infinite.  Needs no cloud.  Does not synchronise.  n_verts or n_faces negative, n_verts above
 *   2^31 - 1, n_faces above 2^29, a NULL buffer with a non-zero size (d_corner_start, d_grad_verts with n_verts > 0; the others with
 *   n_faces > 0): R3G_ERR_INVALID before any launch.  n_verts == 0: success, nothing launched.
 * r3g_cloud_faces_times: milliseconds between HIP events of the last complete calls on this context, ms double [4]: classify,
 *   narrow, wide, gather; -1 for the last while no backward has run.  Without a forward that launched: R3G_ERR_STATE. */
int r3g_cloud_faces(r3g_ctx* ctx, const float* d_verts, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, float* d_dist2,
                    int32_t* d_index, float* d_weights, float* d_diff, int64_t* report, void* stream);
int r3g_cloud_faces_backward(r3g_ctx* ctx, int64_t n_verts, int64_t n_faces, const float* d_grad_dist2, const int32_t* d_index,
                             const float* d_weights, const float* d_diff, const int32_t* d_corner_start, const int32_t* d_corner_ids,
                             float* d_grad_verts, void* stream);
int r3g_cloud_faces_times(r3g_ctx* ctx, double* ms);

/* ---- point clouds: Poisson surface on a uniform lattice -----------------------------------------
 * Oriented points -> an implicit function chi whose level set is the surface (r3g/recon.py runs marching cubes on it).  The
 * lattice has n = 2^depth + 1 nodes per axis over the cube (centre, side), node (i0, i1, i2) stored [i0][i1][i2].  Every value is
 * a pure function of its inputs or an integer sum (csrc/recon_core.h; tests/emu/recon_emu.cpp reproduces each bit on the host).
 * A context keeps the four int64 channels [4][n^3] and the solver's float32 lattices (3 per level); both buffers only grow.  At
 * depth 8 that is 0.54 GB of channels and 0.23 GB of float32 lattices.
 *
 * r3g_recon_splat: d_points, d_normals float32 [n_points][3]; centre double [3] and side are the caller's (host) choice of box.
 *   A point is usable when its coordinates and normal are finite and the normal is non-zero; every usable point adds its trilinear
 *   weights to the 8 nodes of its cell (density channel) and the weights times its unit normal (three vector channels), as int64
 *   sums in units of 2^-30.  A point outside the box counts into the nearest border cell.  d_channels_out (may be NULL): a copy
 *   of the channels, int64 [4][n^3] (density, V0, V1, V2).  *usable_out (may be NULL): usable points.
 *   n_points == 0 or above 2^31 - 1, depth outside [2, 8], a null buffer, a box that is not finite and positive in float32:
 *   R3G_ERR_INVALID before any launch; no usable point: R3G_ERR_INVALID.  A failed call leaves the context without a splat.
 *   Synchronises `stream` (one read-back).
 * r3g_recon_solve: b = div V by central differences (0 on the boundary), then `cycles` V-cycles (in [0, 1000], else
 *   R3G_ERR_INVALID) of geometric multigrid on the 7-point Laplacian with chi = 0 on the boundary, from chi = 0.  d_b_out and
 *   d_chi_out, float32 [n^3], may each be NULL; the context keeps chi for r3g_recon_sample.  Without a successful splat on this
 *   context: R3G_ERR_STATE.  A failed call leaves the context without a solution.  Synchronises `stream`.  Counters
 *   "recon_solves", "recon_cycles".
 * r3g_recon_sample: trilinear sample of field 0 (the density channel) or field 1 (chi) at d_points float32 [n_points][3] into
 *   d_values_out float32 [n_points] (may be NULL).  A point takes part when its coordinates are finite and, where d_normals is
 *   non-NULL, its normal is usable; any other point gets NaN.  *sum_out: the sum of the values that are finite, each rounded to
 *   units of 2^-30, over *count_out points (both may be NULL): an integer sum, so its order decides nothing; it holds while
 *   count * max|value| stays below 2^33.  Without a splat, or field 1 without a solve, on this context: R3G_ERR_STATE; a field other
 *   than 0 or 1, n_points == 0 or above 2^31 - 1, null d_points: R3G_ERR_INVALID, before any launch.  Synchronises `stream`. */
int r3g_recon_splat(r3g_ctx* ctx, const float* d_points, const float* d_normals, int64_t n_points, int depth, const double* centre,
                    double side, int64_t* d_channels_out, int64_t* usable_out, void* stream);
int r3g_recon_solve(r3g_ctx* ctx, int cycles, float* d_b_out, float* d_chi_out, void* stream);
int r3g_recon_sample(r3g_ctx* ctx, int field, const float* d_points, const float* d_normals, int64_t n_points, float* d_values_out,
                     int64_t* sum_out, int64_t* count_out, void* stream);

/* ---- texture stage: native pieces ------------------------------------------------------------
 * SURVEY.md 8(f) rank 3.  Upstream's Hunyuan3DPaintPipeline (reference call site src/2d_to_3d_models/run.py:97, built at
 * :126-128) uses two native extensions, `custom_rasterizer` (CUDA) and `mesh_processor.cpp`, and bakes the generated views
 * into a UV texture in its MeshRender.  These are their gfx950 counterparts; the two diffusion UNets are NOT part of this
 * library.  All buffers are device pointers; images are row-major [H][W][C] float32, row 0 = top.
 *   rasterize     ~ custom_rasterizer.rasterize(pos, tri, (H, W)): pos_clip float32 [V][4], tri int32 [F][3] ->
 *                   findices int32 [H][W] (face + 1, 0 = empty), bary float32 [H][W][3] (perspective-correct).  Pixel
 *                   (ix, iy) samples (ix + 0.5, iy + 0.5) of the screen x = (x/w/2 + 1/2)(W-1) + 1/2; nearest depth wins, equal
 *                   depths go to the smaller face index (result independent of scheduling).  A face is drawn when all its
 *                   w > 0, its screen area is finite and not zero, and its depth z/w * 0.49999 + 1/2 lies in [0, 1].
 *                   COVERAGE is watertight: a sample belongs to a face when its three edge functions have the sign of the
 *                   face's area or are zero (inclusive), and each edge function is evaluated from the edge's two endpoints
 *                   in lexicographic screen (x, y) order, so that the two faces sharing an edge compute the same float with
 *                   opposite signs: no sample on or next to a shared edge is rejected by both.  The barycentrics written are
 *                   clamped at 0 before the perspective division: all three are >= 0 and they sum to 1.  The bounding box is
 *                   clamped in float before it is converted, so a finite coordinate of any size (a vertex with a small
 *                   positive w) is drawn.  With height == 1 or width == 1 the screen scale is 0 and nothing is drawn.
 *   interpolate   ~ custom_rasterizer.interpolate(attr, findices, bary, tri): out[p] = sum_k bary[p][k] attr[tri[f][k]].
 *   view_weight   baking weight of a view: view_weight * cos^power of the view-space normal, 0 below cos_threshold, on
 *                   the silhouette and where the depth jumps by more than depth_edge between 4-neighbours.
 *   bake          scatters a view (image float32 [H][W][3] in [0,1]) into acc uint64 [T][T][4] (zero it first; fixed point,
 *                   integer atomics: exact, order independent); texel = round(uv * (T-1)), v = 0 is the top row.
 *   bake_gather   the same accumulation, texel-centric (what hy3dgen.texgen uses): every texel covered in findices_uv /
 *                   bary_uv (= rasterize() of the mesh in UV space) interpolates its clip position from clip_uv float32
 *                   [Vuv][4] (this view's clip coordinates of the UV vertices), must not lie behind the view's depth
 *                   buffer (depth float32 [H][W] = interpolate() of clip z/w; tolerance depth_eps), takes the weight of the
 *                   pixel it falls into and a bilinear sample of the image.  No atomics; texture as dense as the UV raster.
 *   bake_finalize acc -> texture float32 [T][T][3], mask uint8 [T][T] (1 = painted).
 *   inpaint       ~ mesh_processor.meshVerticeInpaint + the dilation upstream does with cv2: vertex colours from painted
 *                   texels, propagation along mesh edges (weights 1/(d^2 + 1e-6), Jacobi rounds until nothing changes),
 *                   unpainted covered texels from the vertex colours (mask 2), `dilate_iters` steps into empty texels (mask
 *                   3).  findices_uv / bary_uv = rasterize() of the mesh in UV space.  Synchronises the stream.
 * NaN AND OUT-OF-RANGE VALUES are handled by explicit comparisons; no result depends on converting a NaN or an out-of-range
 * float to an integer.  A pixel or texel whose colour, weight or coordinate is NaN contributes NOTHING (neither colour nor
 * weight): a NaN weight (view_weight gives one for a negative cosine with a fractional power) or a weight <= 0 is skipped, a
 * NaN colour channel or bilinear sample skips the whole sample, a NaN texture coordinate, clip position or depth skips it, a
 * corner whose UV is NaN seeds no vertex, an edge whose length is NaN carries no colour.  Finite values are clamped: colours
 * to [0, 1], weights at 65535, texels to [0, T-1] (in float, before the conversion).
 * ZERO SIZES: interpolate and bake with n_pixels == 0 return R3G_OK without a launch (their buffers may then be null);
 * rasterize accepts n_faces == 0 (an empty image).
 * INDEX ARRAYS (tri, uv_tri, pos_tri, findices) must be in range: face ids in [0, n_faces], vertex ids inside their arrays.
 * They are NOT checked on the device; an index out of range reads or writes outside the buffers. */
int r3g_tex_rasterize(r3g_ctx* ctx, const float* d_pos_clip, int64_t n_verts, const int32_t* d_tri, int64_t n_faces, int height,
                      int width, int32_t* d_findices, float* d_bary, void* stream);
int r3g_tex_interpolate(r3g_ctx* ctx, const float* d_attr, int channels, const int32_t* d_tri, const int32_t* d_findices,
                        const float* d_bary, int64_t n_pixels, float* d_out, void* stream);
int r3g_tex_view_weight(r3g_ctx* ctx, const int32_t* d_findices, const float* d_depth, const float* d_normal, int height,
                        int width, float cos_threshold, float depth_edge, float view_weight, float power, float* d_weight,
                        void* stream);
int r3g_tex_bake(r3g_ctx* ctx, const float* d_image, const float* d_weight, const int32_t* d_findices, const float* d_bary,
                 const float* d_uv, const int32_t* d_uv_tri, int64_t n_pixels, int tex_size, uint64_t* d_acc, void* stream);
int r3g_tex_bake_gather(r3g_ctx* ctx, const int32_t* d_findices_uv, const float* d_bary_uv, const float* d_clip_uv,
                        const int32_t* d_uv_tri, int tex_size, const float* d_image, const float* d_weight,
                        const int32_t* d_findices, const float* d_depth, int height, int width, float depth_eps, uint64_t* d_acc,
                        void* stream);
int r3g_tex_bake_finalize(r3g_ctx* ctx, const uint64_t* d_acc, int tex_size, float* d_texture, uint8_t* d_mask, void* stream);
int r3g_tex_inpaint(r3g_ctx* ctx, float* d_texture, uint8_t* d_mask, int tex_size, const int32_t* d_findices_uv,
                    const float* d_bary_uv, const float* d_verts, int64_t n_verts, const int32_t* d_pos_tri, const float* d_uv,
                    const int32_t* d_uv_tri, int64_t n_faces, int dilate_iters, int* rounds_out, void* stream);

/* ---- shape model (DiT + ShapeVAE + DINOv2 conditioner) -----------------------------------------
 * Replaces the modules `Hunyuan3DDiTFlowMatchingPipeline.from_pretrained` instantiates from the
 * checkpoint's config.yaml (reference call sites src/2d_to_3d_models/run.py:122-124,204-206;
 * upstream hy3dgen/shapegen/pipelines.py).  All dimensions are data; head_dim must be 64.
 */
typedef struct r3g_model_config {
    /* denoisers/hunyuan3ddit.py Hunyuan3DDiT */
    int32_t dit_in_channels, dit_context_dim, dit_hidden, dit_heads, dit_depth_double, dit_depth_single,
        dit_mlp_hidden, dit_qkv_bias;
    float dit_time_factor;
    /* autoencoders/model.py ShapeVAE (+ geo_decoder) */
    int32_t vae_num_latents, vae_embed_dim, vae_width, vae_heads, vae_layers, vae_num_freqs, vae_include_pi,
        vae_qkv_bias, vae_qk_norm, vae_mlp_ratio, vae_ln_post;
    float vae_scale_factor;
    /* conditioner.DinoImageEncoder (transformers Dinov2Model, SwiGLU FFN) */
    int32_t cond_image_size, cond_patch, cond_hidden, cond_layers, cond_heads, cond_ffn_hidden;
    float cond_ln_eps;
    /* query points per internal pass of r3g_grid_query (0 = default 131072); NOT upstream's num_chunks:
     * results do not depend on it */
    int32_t grid_chunk;
} r3g_model_config;

/* Allocate the activation arena for this configuration (replaces instantiate_from_config). */
int r3g_model_create(r3g_ctx* ctx, const r3g_model_config* cfg);
/* Register one parameter under its upstream state-dict name ("model.double_blocks.0.img_attn.qkv.weight",
 * "vae.post_kl.bias", "conditioner.main_image_encoder.model.encoder.layer.0.norm1.weight", ...).
 * dtype 0 = float32, 1 = bfloat16.  Matrices: bf16 [rows=N][cols=K], K zero-padded to a multiple of 64;
 * vectors: f32.  The memory stays owned by the caller and must outlive the context.
 * (Replaces load_state_dict of the safetensors checkpoint.) */
int r3g_model_set_tensor(r3g_ctx* ctx, const char* name, const void* d_ptr, int dtype, int64_t rows, int64_t cols);
int r3g_model_set_scalar(r3g_ctx* ctx, const char* name, float value);
/* Give back the device memory the model holds beyond its weights and its arena: the query-side cache of the geo decoder
 * (r3g_grid_query keeps the object-independent half of every grid pass resident, up to the budget of option
 * "geo_q_cache_gb", default 30 % of the device's memory).  The next r3g_grid_query builds it again.  A stage that
 * is about to start another large consumer on the same GPU (texture models, a second process) calls this first.
 * Synchronises the device.  No counterpart upstream (the reference recomputes the query side per chunk). */
int r3g_model_trim(r3g_ctx* ctx);

/* conditioner forward: d_image f32 [3][S][S] already resized/cropped/normalised (ImageEncoder.transform);
 * d_cond_out bf16 [S/14*S/14+1][cond_hidden] = Dinov2Model(...).last_hidden_state (CLS first). */
int r3g_cond_encode(r3g_ctx* ctx, const float* d_image, uint16_t* d_cond_out, void* stream);

/* Hunyuan3DDiT.forward(x, t, contexts={'main': cond}): d_x f32 [B][num_latents][in_channels], d_t f32 [B]
 * (sigma in [0,1]), d_cond bf16 [B][cond_tokens][context_dim] -> d_out f32 like d_x.  B in {1,2}.
 * n_double / n_single < 0 run every block (>= 0: only the first n, for per-block parity tests). */
int r3g_dit_forward(r3g_ctx* ctx, const float* d_x, const float* d_t, const uint16_t* d_cond, float* d_out, int batch,
                    int n_double, int n_single, void* stream);

/* The joint residual stream the preceding r3g_dit_forward(batch, n_double, n_single) left behind, i.e. the input of
 * the next block (or of final_layer): d_out f32 [batch][cond_tokens + num_latents][hidden] in upstream's order
 * cat(cond, latent).  For per-block parity tests: (stream after k+1 blocks) - (stream after k blocks) is block k's
 * branch contribution (hunyuan3ddit.py DoubleStreamBlock / SingleStreamBlock.forward). */
int r3g_dit_stream(r3g_ctx* ctx, float* d_out, int batch, void* stream);

/* The denoising loop of Hunyuan3DDiTFlowMatchingPipeline.__call__ with classifier-free guidance:
 * sigmas = linspace(0,1,steps) (+ FlowMatchEulerDiscreteScheduler shift), per step
 *   v = DiT(cat([x]*2), sigma, d_cond2);  v = v_u + g (v_c - v_u);  x += (sigma_next - sigma) v
 * d_latents f32 [num_latents][in_channels] in/out; d_cond2 bf16 [2][tokens][dim] = [cond, uncond].
 * uncond_uniform != 0 declares that all tokens of the unconditional context are identical (upstream:
 * zeros_like(cond)); they are then carried as ONE token that counts `tokens` times in the softmax -- the same
 * function with 31 % fewer rows in that batch entry (switch "cfg_dedup" of r3g_set_option turns this off). */
int r3g_flow_sample(r3g_ctx* ctx, float* d_latents, const uint16_t* d_cond2, int steps, float guidance_scale,
                    float shift, int uncond_uniform, void* stream);
/* The same loop for n_objects independent objects (upstream: the pipeline's batch dimension when `image` is a list; the
 * reference gets object-level parallelism from its worker pool, src/2d_to_3d_models/run.py:176-193): d_latents f32
 * [n_objects][num_latents][in_channels] in/out, d_cond2 bf16 [n_objects][2][tokens][dim].  With uncond_uniform the objects
 * share every DiT launch (up to 4 per launch; the GEMMs then have enough rows for 256x256 tiles on every layer); each
 * object's result is bit-identical to what r3g_flow_sample gives for it alone. */
int r3g_flow_sample_batch(r3g_ctx* ctx, float* d_latents, const uint16_t* d_cond2, int n_objects, int steps,
                          float guidance_scale, float shift, int uncond_uniform, void* stream);

/* The same loop over an explicit sigma table, and the entry point of GUIDANCE-DISTILLED checkpoints (upstream's subfolders
 * hunyuan3d-dit-v2-0-fast, -turbo, hunyuan3d-dit-v2-mini-turbo; [UPSTREAM-RECALLED]).
 * sigmas: HOST array of n_sigmas = steps + 1 finite values; step i evaluates the model at t = sigmas[i] and updates
 * x += (sigmas[i+1] - sigmas[i]) v; a step with d_sigma = 0 is skipped as in r3g_flow_sample.  r3g_flow_sample and
 * r3g_flow_sample_batch are this function on linspace(0,1,steps) (shifted) + a trailing 1.
 * Which engine runs is decided by what the model holds, not by an option:
 *  - no "model.guidance_in.*" tensor registered: classifier-free guidance exactly as r3g_flow_sample_batch (up to 4 objects per
 *    launch group); with the linspace table the result is bit-identical to it.
 *  - all four of model.guidance_in.{in_layer,out_layer}.{weight,bias} registered: the model is guidance-distilled.
 *    vec = time_in(timestep_embedding(t)) + guidance_in(timestep_embedding(guidance_scale)) -- the guidance scale goes through
 *    the same embedding as t (times time_factor, cos first) --, there is NO CFG batch: one entry per object, conditional context
 *    only, x += d_sigma v.  d_cond2 keeps the [n_objects][2][tokens][dim] layout, its unconditional half is never read, and
 *    uncond_uniform is ignored.  Up to 8 objects share a launch group (same rows per launch as 4 CFG objects); each object's
 *    result is bit-identical to its single-object run.
 *  - a partial set is R3G_ERR_STATE at the first call, naming the missing key.
 * r3g_dit_forward has no guidance input: on a distilled model it evaluates vec = time_in(timestep_embedding(t)) alone (the
 * per-block parity hook).  Not covered: guidance-distilled texture models.  (Top-k KV selection: the "geo_kv_*" options below
 * r3g_grid_query_hier, DESIGN.md section 4d.  Upstream's turbo VAE: a narrow geo decoder, see r3g_vae_decode.) */
int r3g_flow_sample_sigmas(r3g_ctx* ctx, float* d_latents, const uint16_t* d_cond2, int n_objects, const float* sigmas,
                           int n_sigmas, float guidance_scale, int uncond_uniform, void* stream);

/* ShapeVAE.forward(latents / scale_factor) (post_kl + transformer) and the geo decoder's K/V of the
 * result (computed once; upstream recomputes them for every chunk).  d_z_out (optional) f32
 * [num_latents][width] receives the decoded latents.
 * NARROW GEO DECODER (upstream's turbo VAE, geo_decoder_downsample_ratio; [UPSTREAM-RECALLED], DEFINED in DESIGN.md section 4e).
 * r3g_model_config has no field for it: the registered tensors decide.  width_g = rows of "vae.geo_decoder.query_proj.weight",
 * heads_g = width_g / 64, the MLP's hidden size = rows of its mlp.c_fc.weight.  width_g == vae_width is the ordinary decoder.
 * Otherwise "vae.geo_decoder.latents_proj.{weight,bias}" ([width_g][vae_width], with bias) must be registered: it is applied to the
 * transformer's output before the decoder's ln_2, and every tensor of the decoder has width_g where it had vae_width.  A width_g
 * that is no multiple of 64 or exceeds vae_width is R3G_ERR_INVALID (the message names the tensor); a missing latents_proj is
 * R3G_ERR_STATE.  r3g_grid_query, r3g_grid_query_points, r3g_grid_query_hier and top-k KV selection work unchanged on it; with
 * option "geo_fp8" != 0 every grid query of a narrow decoder is R3G_ERR_INVALID. */
int r3g_vae_decode(r3g_ctx* ctx, const float* d_latents, float* d_z_out, void* stream);

/* VanillaVolumeDecoder: occupancy logits of dense grid points [start, start+count) of the (R+1)^3 grid
 * (point index = (i*(R+1)+j)*(R+1)+k, coordinates np.linspace(-bound, bound, R+1)) written to
 * d_grid[start ...], fp32.  Needs a preceding r3g_vae_decode. */
int r3g_grid_query(r3g_ctx* ctx, double bound, int octree_resolution, float* d_grid, int64_t start, int64_t count,
                   void* stream);

/* ---- hierarchical volume decoding (upstream: pipeline.enable_flashvdm(); opt-in, the default stays r3g_grid_query) ------------
 * The dense decoder evaluates all (R+1)^3 points although marching cubes only reads the cells the surface passes through.  The
 * hierarchical decoder evaluates a coarse lattice densely and, level by level, only the points near the surface of the level
 * below.  It is DEFINED here and in DESIGN.md ("Hierarchical volume decoding"); it is modelled on upstream's hierarchical
 * decoder but not pinned to it (parity-unpinned, like the rest of the VAE).
 *   levels(R, min_resolution): start from R; while the value is even and its half is >= min_resolution, append the half;
 *   coarsest first (256 -> 64, 128, 256; an odd R -> R alone: the dense decoder).  Level l has R_l + 1 points per axis; fine
 *   index 2p is coarse point p.
 *   From the complete grid G of the level below, the iso level and a band:  s(p) = G(p) > level (as a double, NaN: false -- the
 *   marching-cubes inside test);  near(p) = some 6-neighbour q inside the grid has s(q) != s(p);  cand(p) = near(p) or
 *   |G(p) - level| < band (double arithmetic, NaN: false);  e = 0 when the level being built is the finest, else 1;  C = cand
 *   dilated e times by the 3x3x3 box;  F = the seed F0(2p) = C(p) dilated 2 - e times on the fine lattice (clipped to the grid).
 *   The active points are F in ascending linear index; the decoder is evaluated at each of them with that level's own
 *   coordinates; every other fine point q takes G(q >> 1 per axis).
 * r3g_hier_select: steps above for one level on ANY coarse fp32 grid [n_coarse]^3 (2 <= n_coarse <= 645; no model needed):
 *   keeps the mask and its rank table in the context (like r3g_mc_count) and returns the number of active points of the
 *   (2 n_coarse - 1)^3 fine lattice in *count.  Synchronous: one 8-byte read-back.
 * r3g_hier_indices: the ascending int32 linear indices of the preceding select -> d_idx_out[count].
 * r3g_hier_merge: d_fine_out[(2 n_coarse - 1)^3] (16-byte aligned) = d_values[rank] at the active points (d_values in the order
 *   of r3g_hier_indices), the floor parent of d_coarse everywhere else.
 * r3g_grid_query_points: the geo decoder at `count` listed points (linear indices into the (R+1)^3 lattice, any order, int32)
 *   -> d_values[count].  Same launches as r3g_grid_query per pass: a point's logit equals the dense grid's bit for bit.  Never
 *   reads, builds or re-keys the query-side cache of r3g_grid_query.  Needs a preceding r3g_vae_decode.
 * r3g_grid_query_hier: the whole decode into d_grid [(R+1)^3] (16-byte aligned): level 0 densely, then select / indices / listed
 *   points / merge per level.  Points evaluated at the finest level hold exactly the dense decoder's values; the others hold a
 *   coarser level's value of their floor parent.  One read-back per level.  The levels below the finest and the listed points
 *   stay away from the query-side cache (a hierarchical object between two dense ones leaves it as it was); a single-level
 *   decode (odd R, or R / 2 < min_resolution) IS r3g_grid_query.  stats (optional, n_stats >= 4 + 2 * levels; one more
 *   read-back): [0] levels, [1] points evaluated in total, [2] (R+1)^3, [3] unsafe cells -- cells of the result whose corners
 *   are not all on one side of mc_level and not all active (their triangles rest on a filled value) --, then per level
 *   [4 + 2l] R_l and [5 + 2l] points evaluated.
 * Both grid entry points refuse the fp8 mode (option "geo_fp8" != 0) with R3G_ERR_INVALID: it is not covered by the bit-equality
 * tests of the listed-points path.
 * "The dense grid's bit for bit" holds for EXACT cross-attention (the default).  Under top-k KV selection (below) the keys a point
 * attends to depend on the group of consecutive points it is evaluated with: the groups of a dense pass and of a list differ, so a
 * listed point's logit is no longer the dense grid's, and the hierarchical decoder's grid is not the dense decoder's at the points
 * it evaluates. */
int r3g_hier_select(r3g_ctx* ctx, const float* d_coarse, int n_coarse, double level, double band, int is_finest, int64_t* count,
                    void* stream);
int r3g_hier_indices(r3g_ctx* ctx, int32_t* d_idx_out, void* stream);
int r3g_hier_merge(r3g_ctx* ctx, const float* d_coarse, const float* d_values, float* d_fine_out, void* stream);
int r3g_grid_query_points(r3g_ctx* ctx, double bound, int octree_resolution, const int32_t* d_idx, int64_t count, float* d_values,
                          void* stream);
int r3g_grid_query_hier(r3g_ctx* ctx, double bound, int octree_resolution, double mc_level, double band, int min_resolution,
                        float* d_grid, int64_t* stats, int n_stats, void* stream);

/* ---- adaptive top-k KV selection in the geo decoder (upstream: FlashVDM's adaptive_kv_selection; opt-in, the default is exact) --
 * [UPSTREAM-RECALLED], parity-unpinned; DEFINED in DESIGN.md section 4d.  An approximation: per group of `geo_kv_group` consecutive
 * points of a pass (the evaluation order of r3g_grid_query / r3g_grid_query_points; the last group of a pass may be shorter) and
 * per head, every key is scored by q-bar . k in fp32 -- q-bar the mean of the group's query rows r with r % geo_kv_stride == 0, the
 * bf16 rows the attention kernel reads --, the k keys of largest score are kept (equal scores: the lower key index; NaN below
 * every number) in ascending key index, and the group's attention runs over those keys only.  With k >= num_latents the selection
 * is the identity and the logits equal the exact path's bit for bit.  Everything around the attention call, the query-side cache
 * included, is unchanged.  The error against exact attention depends on how peaked the checkpoint's attention is: it is
 * reported (tools/bench_kvsel.py, profiles/kvsel.md), not bounded.
 * Options of r3g_set_option: "geo_kv_topk" (0 default: exact | k > 0: keys kept, clamped to num_latents | -1: upstream's rule, 1024
 * of 3072, 256 of 512, otherwise num_latents / 3; below -1 refused), "geo_kv_group" (8192; a multiple of 256, at least 256, anything
 * else is refused), "geo_kv_stride" (64; below 1 is refused).  A refused value is R3G_ERR_INVALID and changes nothing.  With option
 * "geo_fp8" != 0 every grid query in top-k mode is R3G_ERR_INVALID.  Counter "geo_kv_groups": (group, head) selections so far.
 * r3g_kv_selection_last: the index table int32 [groups][heads][k] of the LAST pass evaluated in top-k mode -> d_idx (capacity in
 * entries; d_idx may be null to read the shape alone); groups in the pass's order, a tail group last.  R3G_ERR_STATE when there
 * is none.
 * r3g_kv_selection_operands: what that table was selected from -- the pass's Q rows bf16 [heads][lq_pad][64] (lq valid; q-normed,
 * pre-scaled, as the attention kernel reads them) -> d_q and the object's K bf16 [heads][lk_pad][64] -> d_k (capacities in
 * elements; either pointer may be null, the four shape outputs too).  Valid until the next grid query, r3g_vae_decode or
 * r3g_model_trim.  For tests: r3g_op_kv_select on these operands reproduces the table. */
int r3g_kv_selection_last(r3g_ctx* ctx, int32_t* d_idx, int64_t capacity, int* groups, int* heads, int* k, void* stream);
int r3g_kv_selection_operands(r3g_ctx* ctx, uint16_t* d_q, int64_t q_capacity, uint16_t* d_k, int64_t k_capacity, int* lq, int* lq_pad,
                              int* lk, int* lk_pad, void* stream);

/* ---- texture stage: UNet blocks (first slice) -------------------------------------------
 * The two diffusion models behind upstream's Hunyuan3DPaintPipeline.__call__ (reference call site
 * src/2d_to_3d_models/run.py:97; built at :126-128, :207-209) are diffusers UNet2DConditionModels on the Stable-Diffusion-2.1
 * layout.  These entry points are their building blocks on gfx950 -- ResnetBlock2D, Transformer2DModel
 * (use_linear_projection, one BasicTransformerBlock: self-attention, cross-attention over the context, GEGLU feed-forward),
 * Downsample2D / Upsample2D, the compositions CrossAttnDownBlock2D / UNetMidBlock2DCrossAttn, and the whole
 * UNet2DConditionModel.forward (r3g_unet_forward); the VAE, the schedulers, the context encoders and upstream's multiview /
 * reference attention extensions are NOT part of this library yet (the stage keeps reporting where its colours come from).
 * Activations are rows: f32 [height*width][channels] (NHWC: a pixel's channels contiguous; channels % 64 == 0, head dim
 * 64), the context bf16 [tokens][ctx_dim], the time embedding f32 [temb_dim] (the output of the UNet's time_embedding MLP).
 * Weights are registered under diffusers' state-dict names below `prefix` ("down_blocks.0", "mid_block", ...):
 *   3x3 convolutions bf16 [C_out][9 C_in] with column (ky*3 + kx)*C_in + c (a re-layout of torch's [C_out][C_in][3][3]),
 *   linear layers bf16 [N][K], vectors f32; fused projections registered as "<block>.attn1.to_qkv.weight" = rows of to_q, to_k,
 *   to_v and "<block>.attn2.to_kv.weight" = per head its 64 rows of to_k then its 64 rows of to_v (pure re-layouts, done by
 *   r3g/unet.py).  All calls enqueue on `stream` and return. */
typedef struct r3g_unet_config {
    int32_t max_hw;         /* largest height*width an entry point will see */
    int32_t max_channels;   /* largest channel count (multiple of 64, <= 2048) */
    int32_t temb_dim;       /* 1280 for SD 2.1 */
    int32_t ctx_dim;        /* cross_attention_dim: 1024 for SD 2.1 */
    int32_t ctx_tokens;     /* most context tokens (77 for CLIP text) */
    int32_t groups;         /* norm_num_groups: 32 */
    float resnet_eps;       /* GroupNorm eps of the resnets: 1e-5 (Transformer2DModel's norm uses 1e-6, its LayerNorms 1e-5) */
    /* block structure, for r3g_unet_forward only (0 levels: building blocks only): SD 2.1 = 4 levels (320, 640, 1280, 1280),
     * 2 layers per block, 4 -> 4 channels.  max_channels must cover the widest concatenation of the up path (2560) */
    int32_t n_levels, layers_per_block, in_channels, out_channels;
    int32_t block_out_channels[4];
} r3g_unet_config;
int r3g_unet_create(r3g_ctx* ctx, const r3g_unet_config* cfg);
int r3g_unet_set_tensor(r3g_ctx* ctx, const char* name, const void* d_ptr, int dtype, int64_t rows, int64_t cols);
/* ResnetBlock2D.forward(x, temb) -> d_out f32 [height*width][c_out] (may alias d_x when c_in == c_out) */
int r3g_unet_resnet(r3g_ctx* ctx, const char* prefix, const float* d_x, int height, int width, int c_in, int c_out,
                    const float* d_temb, float* d_out, void* stream);
/* Transformer2DModel.forward(x, encoder_hidden_states), in place on d_x */
int r3g_unet_transformer(r3g_ctx* ctx, const char* prefix, float* d_x, int height, int width, int channels, const uint16_t* d_ctx,
                         int tokens, void* stream);
/* Downsample2D.forward: conv 3x3, stride 2, padding 1 -> d_out f32 [(height+1)/2 * (width+1)/2][channels] */
int r3g_unet_downsample(r3g_ctx* ctx, const char* prefix, const float* d_x, int height, int width, int channels, float* d_out,
                        void* stream);
/* CrossAttnDownBlock2D.forward: `layers` x (resnet, transformer) [+ downsample].  d_states f32 [layers][height*width][c_out]
 * receives every layer's hidden state (diffusers' output_states: the skip connections); d_out the downsampled result. */
int r3g_unet_down_block(r3g_ctx* ctx, const char* prefix, const float* d_x, int height, int width, int c_in, int c_out,
                        const float* d_temb, const uint16_t* d_ctx, int tokens, int layers, int add_downsample, float* d_states,
                        float* d_out, void* stream);
/* UNet2DConditionModel.forward(sample, timestep, encoder_hidden_states) on the SD-2.1 layout (CrossAttnDownBlock2D x (n-1) +
 * DownBlock2D | UNetMidBlock2DCrossAttn | UpBlock2D + CrossAttnUpBlock2D x (n-1); conv_in / time_embedding / conv_norm_out /
 * conv_out under diffusers' names; "conv_in.weight" registered with its input channels zero-padded to 64):
 * d_sample f32 [height*width][in_channels] -> d_out f32 [height*width][out_channels]; height, width divisible by 2^(n-1). */
int r3g_unet_forward(r3g_ctx* ctx, const float* d_sample, int height, int width, float timestep, const uint16_t* d_ctx, int tokens,
                     float* d_out, void* stream);
/* ---- several samples per call and upstream's 2.5D transformer blocks: the multiview UNet of the texture stage ----
 * [UPSTREAM-RECALLED] hy3dgen/texgen/hunyuanpaint/unet/modules.py: UNet2p5DConditionModel wraps an SD-2.1 UNet2DConditionModel;
 * every BasicTransformerBlock becomes a Basic2p5DTransformerBlock with two more attentions on norm1's output --
 * attn_multiview (self-attention over the tokens of ALL views of the object as one sequence, scaled by mva_scale) and
 * attn_refview (every view's tokens attend to the normalised hidden states a separate "reference" UNet pass over the input
 * image has kept per block, scaled by ref_scale) --, conv_in takes 12 channels (latent | normal map latent | position map
 * latent) and an nn.Embedding over camera indices is added to the time embedding (class_labels).
 * Samples are stacked as rows: d_sample f32 [n_views][height*width][in_channels], d_out likewise; r3g_unet_create's max_hw
 * is then the largest n_views*height*width, ctx_tokens at least the number of reference tokens.  Extra tensors
 * (r3g_unet_set_tensor): "<...>.transformer_blocks.0.attn_multiview.to_qkv.weight" ([3C][C]: to_q | to_k | to_v),
 * ".attn_multiview.to_out.0.{weight,bias}", ".attn_refview.to_q.weight", ".attn_refview.to_kv.weight" (per head 64 k rows,
 * 64 v rows), ".attn_refview.to_out.0.{weight,bias}", "class_embedding.weight" (f32 [classes][temb_dim]), and per transformer
 * "cond:<transformer prefix>" = the reference pass's kept states (bf16 [reference tokens][C], from r3g_unet_condition of the
 * context that ran the reference pass).  Blocks whose 2.5D weights are not registered run as the plain block.
 * flags: 1 = keep norm1's output of every transformer ("w" mode, the reference pass), 2 = run attn_refview where its weights
 * and "cond:" tensor exist ("r" mode), 4 = the n_views samples are the two evaluations of one classifier-free-guidance step in
 * ONE launch set (round 5; n_views even, not with flag 1): samples [0, n_views/2) are the conditional evaluation -- context rows
 * [0, tokens) of d_ctx, attn_refview under flag 2 --, samples [n_views/2, n_views) the unconditional one -- context rows
 * [tokens, 2 tokens) of d_ctx (bf16 [2 tokens][ctx_dim]), no attn_refview --, and attn_multiview's sequence is one HALF's
 * views; every sample's result equals its two-call result up to the order of fp32 additions in the split-K convolutions.
 * max_hw must then hold n_views*height*width rows.  class_labels: host array [n_views] or NULL. */
int r3g_unet_forward_mv(r3g_ctx* ctx, const float* d_sample, int height, int width, float timestep, const uint16_t* d_ctx, int tokens,
                        int n_views, const int32_t* class_labels, int flags, float mva_scale, float ref_scale, float* d_out,
                        void* stream);
/* one Transformer2DModel with the 2.5D block, in place on d_x f32 [n_views][height*width][channels] */
int r3g_unet_transformer_mv(r3g_ctx* ctx, const char* prefix, float* d_x, int height, int width, int channels, const uint16_t* d_ctx,
                            int tokens, int n_views, int flags, float mva_scale, float ref_scale, void* stream);
/* what a pass with flag 1 kept for the transformer `prefix` ("down_blocks.0.attentions.1", "mid_block.attentions.0", ...):
 * bf16 [rows = samples*height*width][cols = channels], owned by the context, valid until its next pass with flag 1 */
int r3g_unet_condition(r3g_ctx* ctx, const char* prefix, const void** d_ptr, int64_t* rows, int64_t* cols);
/* UNetMidBlock2DCrossAttn.forward: resnet, transformer, resnet -> d_out f32 [height*width][channels] */
int r3g_unet_mid_block(r3g_ctx* ctx, const char* prefix, const float* d_x, int height, int width, int channels,
                       const float* d_temb, const uint16_t* d_ctx, int tokens, float* d_out, void* stream);

/* ---- the SD-family VAE (diffusers AutoencoderKL) on the same blocks ------------------------------
 * Replaces, inside upstream's texture pipelines (behind reference src/2d_to_3d_models/run.py:97), `vae.encode(image)` /
 * `vae.decode(latents)` of the delight and multiview diffusion models.  The context is one created by r3g_unet_create with
 * block_out_channels = the ENCODER's order (128, 256, 512, 512), layers_per_block 2, in_channels = latent channels (4),
 * out_channels = image channels (3), groups 32, resnet_eps 1e-6; weights registered with r3g_unet_set_tensor under diffusers'
 * names ("encoder.down_blocks.0.resnets.0.conv1.weight", "decoder.mid_block.attentions.0.to_q.weight", "quant_conv.weight",
 * "post_quant_conv.weight", ...), 3x3 convolutions re-laid as for the UNet, conv_in's input channels and the 1x1 convolutions'
 * K zero-padded to 64, conv_out / quant_conv / post_quant_conv rows zero-padded to a multiple of 4 (python: r3g.unet).
 * The mid block's single-head attention (head dim = channels) is two GEMMs around a row softmax; height*width of the
 * latent grid must be a multiple of 64. */
/* AutoencoderKL.decode(z).sample: d_latent f32 [height*width][latent channels] (already divided by the scaling factor) ->
 * d_image f32 [(8 height)(8 width)][4] (channels 0..2 = RGB in [-1, 1] nominally, channel 3 = 0) */
int r3g_aekl_decode(r3g_ctx* ctx, const float* d_latent, int height, int width, float* d_image, void* stream);
/* AutoencoderKL.encode(x).latent_dist parameters: d_image f32 [height*width][image channels] -> d_moments f32
 * [(height/8)(width/8)][2 latent channels] = (mean | log-variance); the distribution's mode is the mean */
int r3g_aekl_encode(r3g_ctx* ctx, const float* d_image, int height, int width, float* d_moments, void* stream);

/* ---- sampling loops of upstream's diffusion pipelines (the delighting StableDiffusionInstructPix2PixPipeline and the
 * multiview pipeline, both with an EulerAncestralDiscreteScheduler; [UPSTREAM-RECALLED] hy3dgen/texgen/utils/dehighlight_utils.py,
 * hy3dgen/texgen/hunyuanpaint/pipeline.py) around r3g_unet_forward / r3g_unet_forward_mv: the elementwise steps diffusers runs
 * between UNet evaluations.  Stateless (no context). */
/* d_out f32 [pixels][channels + cond_channels] = (d_latent[p] / sqrt(sigma^2 + 1) | d_cond[p]):
 * scheduler.scale_model_input(latents, t) and torch.cat([latents, conditioning latents], dim=1) on rows (InstructPix2Pix: the image
 * latents; the multiview pipeline: the normal- and position-map latents of the view) */
int r3g_sched_model_input(const float* d_latent, int channels, const float* d_cond, int cond_channels, int64_t pixels, float sigma,
                          float* d_out, void* stream);
/* the InstructPix2Pix case: cond_channels = channels */
int r3g_sched_pix2pix_input(const float* d_latent, const float* d_image_latent, int channels, int64_t pixels, float sigma,
                            float* d_out, void* stream);
/* classifier-free guidance: d_out[i] = d_uncond[i] + guidance_scale (d_cond[i] - d_uncond[i]) */
int r3g_sched_cfg_combine(const float* d_uncond, const float* d_cond, int64_t n, float guidance_scale, float* d_out, void* stream);
/* EulerAncestralDiscreteScheduler.step in place on d_sample f32 [n]: prediction_type 0 epsilon | 1 v_prediction;
 * sigma_up^2 = sigma_to^2 (sigma_from^2 - sigma_to^2) / sigma_from^2, sigma_down^2 = sigma_to^2 - sigma_up^2,
 * sample += (sample - x0) / sigma_from * (sigma_down - sigma_from) + d_noise * sigma_up */
int r3g_sched_euler_ancestral_step(float* d_sample, const float* d_model_out, const float* d_noise, int64_t n, float sigma_from,
                                   float sigma_to, int prediction_type, void* stream);

/* ---- single kernels, for parity tests through the ABI ------------------------------------------ */
/* C = epilogue(A[m][k] . W[n][k]^T + bias); epilogue: 0 bf16, 1 bf16 gelu(tanh), 2 bf16 gelu(erf),
 * 3 f32 C += gate*(..), 4 f32, 6 bf16 C = bf16(C + gate*(..)), 8 the same in fp16 (the sum formed in fp32; gate null: 1).  Any other
 * epilogue is R3G_ERR_INVALID: 5 and 9-11 need operands this entry point cannot carry, 7 belongs to r3g_op_gemm_fp8_e4m3.
 * Shapes: m >= 0 (0: nothing is launched), k % 64 == 0, n % 4 == 0.  Operands: a and w are staged 16 bytes at a time -- lda % 8 == 0,
 * ldw % 8 == 0, both >= k, d_a and d_w 16-byte aligned; d_bias and d_gate (either may be null) 16-byte aligned, n floats each.
 * Output: the kernels store four consecutive columns at a time on their narrowest path, so ldc % 4 == 0, ldc >= n, and d_c aligned to
 * four elements: 8 bytes for the 16-bit outputs (0, 1, 2, 6, 8), 16 bytes for the fp32 ones (3, 4).  With n % 8 == 0, ldc % 8 == 0 and a
 * 16-byte aligned d_c the 16-bit outputs leave through the LDS transpose in 16-byte stores instead (same values).  Nothing outside
 * [m) x [n) of C is written; rows past m and columns past n of a, w, bias and gate are never read.  A violation is R3G_ERR_INVALID
 * (tests/test_gemm_edges_gpu.py runs every tile kernel at the loosest alignment this admits). */
int r3g_op_gemm(const uint16_t* d_a, int64_t lda, const uint16_t* d_w, int64_t ldw, const float* d_bias, void* d_c,
                int64_t ldc, const float* d_gate, int m, int n, int k, int epilogue, int use_lds_dma, void* stream);
/* r3g_op_gemm for the fp32 epilogues (3, 4) with the caller's split-K workspace d_ws (ws_elems floats), as the texture UNets' 3 x 3
 * convolutions launch it (csrc/unet.cpp: u_conv3x3): a problem of at most 256 tiles of 128 x 128 with k >= 2048 runs as S slices of k
 * -- the S batches of one launch of the 128 x 128 kernel into d_ws [S][m][n] -- that a second kernel adds in the order 0 .. S-1
 * before bias / gate / residual (S = the largest divisor of k / 64 with S * tiles <= 512 and >= 8 k-steps per slice; two slices only from k = 4096).  No atomics:
 * the result is a pure function of the operands and (m, n, k).  *slices (may be null) = S, 1 = the ordinary launch. */
int r3g_op_gemm_splitk(const uint16_t* d_a, int64_t lda, const uint16_t* d_w, int64_t ldw, const float* d_bias, float* d_c, int64_t ldc,
                       const float* d_gate, int m, int n, int k, int epilogue, float* d_ws, int64_t ws_elems, int* slices,
                       void* stream);
/* One 3 x 3 convolution of the texture models through the dispatch their own blocks use (csrc/unet.cpp: conv3x3_run), on caller-owned
 * operands (tests/test_conv_edges_gpu.py).  d_x bf16 [nb][height*width][cin] (samples stacked as rows, a pixel's channels contiguous),
 * d_w bf16 [cout][ky][kx][cin] (row stride 9 cin), d_bias f32 [cout] or null -> d_c f32 [nb*Ho*Wo][ldc], Ho = (height + pad - 2) / stride
 * + 1, Wo likewise; epilogue 4: c = conv + bias, 3: c += conv + bias.  stride 1 | 2; pad 1: zero padding all round, pad 0: one row below
 * and one column to the right only, F.pad(x, (0, 1, 0, 1)).  A window never reads the neighbouring sample.
 * The launch is conv_gemm_kernel (the 128 x 128 kernel gathers its A operand itself, taps outside the image from a page of zeros the
 * context owns) while "conv_implicit" is on, LDS-DMA staging and the automatic tile rule are in force and that rule does not give the
 * problem to the 256 x 256 kernels; otherwise im2col3x3_kernel writes d_col [nb*Ho*Wo][9 cin] (col_elems elements, caller-owned) and the
 * ordinary GEMM runs on it -- same bits.  Either form splits k as r3g_op_gemm_splitk states when d_ws (ws_elems floats, caller-owned)
 * holds S * nb*Ho*Wo * cout floats; d_ws null or too small: one launch walks all of k.  *implicit (may be null) = 1 when
 * conv_gemm_kernel ran, *slices (may be null) = the slices the launch really used.
 * Contract, checked; a violation is R3G_ERR_INVALID with nothing launched or written: ctx, d_x, d_w, d_c non-null; nb, height, width
 * >= 1 (nb * height * width < 2^27); height + pad >= 2 and width + pad >= 2 (a window that lies in the padding alone is what PyTorch
 * refuses too); cin % 64 == 0; cout % 4 == 0; ldc % 4 == 0, ldc >= cout; d_x, d_w, d_c, d_bias, d_col and d_ws 16-byte aligned;
 * epilogue 3 or 4; a launch that needs the im2col matrix while d_col is null or col_elems < nb*Ho*Wo * 9 cin.  Nothing outside
 * [nb*Ho*Wo) x [cout) of d_c, past nb*Ho*Wo * 9 cin elements of d_col or past S * nb*Ho*Wo * cout floats of d_ws is written; nothing
 * in front of d_x, past its nb * height * width rows or past row cout of d_w is read. */
int r3g_op_conv3x3(r3g_ctx* ctx, const uint16_t* d_x, int nb, int height, int width, int cin, int stride, int pad, const uint16_t* d_w,
                   int cout, const float* d_bias, float* d_c, int64_t ldc, int epilogue, uint16_t* d_col, int64_t col_elems, float* d_ws,
                   int64_t ws_elems, int* implicit, int* slices, void* stream);
/* Nearest-neighbour 2 x upsampling in front of Upsample2D's convolution (upsample2x_kernel): d_x f32 [height][width][channels] -> d_y
 * bf16 [2 height][2 width][channels], y[oy][ox] = bf16(x[oy / 2][ox / 2]) rounded to nearest even.  channels % 4 == 0, height, width
 * >= 1, d_x 16-byte and d_y 8-byte aligned, both non-null; a violation is R3G_ERR_INVALID with nothing written. */
int r3g_op_upsample2x(const float* d_x, int height, int width, int channels, uint16_t* d_y, void* stream);
/* softmax(Q K^T / 8) V for head_dim 64: Q bf16 [B][H][lq_pad][64] (plain q: this entry point folds the softmax scale
 * in itself), K bf16 [B][H][lk_pad][64], Vt bf16 [B][H][64][lk_pad] -> O bf16 [B][lq][H*64].
 * Vt holds V transposed with the keys of each row in the kernel's operand order: inside every aligned group of 16 keys
 * the two middle 4-key blocks are swapped (key 8g+4h+e at position 8h+4g+e; python: r3g.layout.make_vt). */
int r3g_op_attention(const uint16_t* d_q, const uint16_t* d_k, const uint16_t* d_vt, uint16_t* d_o, int batch, int heads,
                     int lq, int lq_pad, int lk, int lk_pad, int shared_kv, int use_lds_dma, void* stream);
/* The two steps of top-k KV selection (above) on caller-owned operands.  kv_select: Q bf16 [heads][lq_pad][64], K bf16
 * [heads][lk_pad][64] -> d_idx int32 [ceil(lq / group)][heads][topk], ascending per (group, head); 1 <= topk <= lk <= 15360.
 * kv_gather: K as before, Vt bf16 [heads][64][lk_pad] in the attention kernel's key order (r3g_op_attention) -> d_k_out bf16
 * [groups][heads][kpad][64] = K[idx] and d_vt_out bf16 [groups][heads][64][kpad] = the transposed V[idx] with compact key j at the
 * kernel's position of j; kpad = topk rounded up to 64, padded keys zero: the operands of r3g_op_attention(batch = groups,
 * shared_kv = 0).  kv_gather is synchronous (it makes its own row-major copy of V). */
int r3g_op_kv_select(const uint16_t* d_q, int lq, int lq_pad, const uint16_t* d_k, int lk, int lk_pad, int heads, int group, int stride,
                     int topk, int32_t* d_idx, void* stream);
int r3g_op_kv_gather(const uint16_t* d_k, const uint16_t* d_vt, int lk, int lk_pad, int heads, const int32_t* d_idx, int groups, int topk,
                     uint16_t* d_k_out, uint16_t* d_vt_out, void* stream);
/* The fused tail of a narrow geo decoder of width 256 (csrc/geo_narrow.hip) on caller-owned operands: d_cat
 * (the attention output) and d_x0 (the start of the residual stream) bf16 [n][256]; weights bf16 row-major d_w_proj [256][256],
 * d_w_fc [hidden][256], d_w_fp [256][hidden], hidden 256 | 512 | 1024; biases and LayerNorm vectors f32; d_lnpost_w / d_lnpost_b
 * both null: no ln_post.  d_logits f32 [n] = output_proj(ln_post(x1 + mlp(ln_3(x1)))), x1 = x0 + c_proj(cat).  Rows past n are
 * neither read nor written.  Synchronous (it packs the weights into its own scratch buffer per call). */
int r3g_op_geo_tail(const uint16_t* d_cat, const uint16_t* d_x0, int n, int hidden, const uint16_t* d_w_proj, const float* d_b_proj,
                    const float* d_ln3_w, const float* d_ln3_b, const uint16_t* d_w_fc, const float* d_b_fc, const uint16_t* d_w_fp,
                    const float* d_b_fp, const float* d_lnpost_w, const float* d_lnpost_b, const float* d_out_w, float out_b,
                    float* d_logits, void* stream);
/* The row kernels of the hot path, one launch each on caller-owned operands (tests/test_row_kernels_gpu.py,
 * tests/test_tex_row_kernels_gpu.py).  Every entry point checks the contract stated here -- the model's own launches meet it by
 * construction, the launchers check only part of it -- and a violation is R3G_ERR_INVALID with nothing written.  Common to all:
 * rows >= 1 (l, batch, heads, nb likewise), every pointer named as required non-null, a row stride at least the row's width.
 *
 * layernorm: y bf16 [rows][c] = ((x - mean) rstd (w ? w[c] : 1) + (b ? b[c] : 0)) (1 + scale[batch][c]) + shift[batch][c], every product and
 *   sum rounded on its own, biased variance, rstd = 1 / sqrt(var + eps).  x_format 0 f32 | 1 bf16 | 2 fp16 (16-bit rows: c % 256 == 0);
 *   c % 64 == 0, 64 <= c <= 2048.  Row r is row r % rows_per_batch of batch r / rows_per_batch: x at batch * x_batch_stride + row * ldx,
 *   y likewise (y batches must not overlap), scale / shift (each may be null) at batch * mod_stride.  Rows in [seg2_row0, seg2_row1) take
 *   d_scale2 / d_shift2 (both required then) instead.  16-bit rows, and f32 rows with c % 256 == 0, ldx % 4 == 0 and ldy % 4 == 0, run on
 *   the row-in-registers kernel, which moves four elements per access: ldx, x_batch_stride, ldy, y_batch_stride, mod_stride % 4 == 0, x
 *   and y aligned to four elements, the six vectors to 16 bytes.  Any other f32 row runs on the scalar kernel (no alignment demands).
 *   d_y8 != null: INSTEAD of y, OCP e4m3 bytes [rows][ldy8] and d_y_scale f32 [rows] (amax / 448 of the finished row, floored at 2^-126
 *   as r3g_op_quant_fp8 states, 1 for an all-zero row; round to nearest even).  That form indexes its outputs by the launch row, so it takes one batch only: d_y null, ldy = 0, both
 *   batch strides 0, rows_per_batch >= rows, c % 256 == 0 on the row-in-registers kernel, ldy8 % 4 == 0, d_y8 4-byte aligned.
 * ln_dot: d_out f32 [rows] = (do_ln ? LN(x) (lnw, lnb: both or neither) : x) . w + b; x f32 or bf16 (x_bf16 1: c % 256 == 0), c as above;
 *   f32 rows with c % 256 == 0 and ldx % 4 == 0, and all bf16 rows, move four elements per access (alignment as for layernorm).
 * qkv_split: src bf16 [batch][l][ld] -> Q bf16 [batch][heads][lq_pad][64], K bf16 [batch][heads][lk_pad][64], Vt bf16
 *   [batch][heads][64][lk_pad] in the attention kernel's key order (r3g_op_attention), token t at destination row dst_row0 + t.  Head h of
 *   q | k | v sits at columns x_off + h * head_stride .. + 63; x_off = -1 with a null destination: absent.  norm 0 none | 1 RMSNorm | 2
 *   LayerNorm over the 64 columns of q and of k (weights optional, biases for 2 only), q then times q_scale (0: 1).  dst_row0 % 64 == 0,
 *   lq_pad % 128 == 0, lk_pad % 64 == 0, dst_row0 + l <= the pad of every destination given.  V^T columns of the last 64-token block
 *   past l are written as zeros; nothing else outside the call's rows and columns is written.
 * group_norm: x f32 [nb][rows][c] -> y bf16 [nb][rows][c] = act(((x + addv[sample]) - mean) rstd gamma + beta), statistics per (sample,
 *   group) over rows x c / groups values, biased; act = SiLU when do_silu.  c % 4 == 0, c <= 3072, 1 <= groups <= 256, c % groups == 0;
 *   addv (may be null) f32 [nb][add_stride], add_stride % 4 == 0; 16-byte aligned x / gamma / beta / addv, 8-byte aligned y.
 *   Synchronous (it allocates the partial-sum workspace per call).
 * softmax_rows: P bf16 [rows][n] = softmax(scale * S[r][:]), S f32; n % 4 == 0, lds % 4 == 0, ldp % 4 == 0, S 16-byte and P 8-byte
 *   aligned, scale > 0 (the kernel scales the maximum of the raw scores).
 * geglu: out bf16 [rows][f] = in[r][c] * gelu_erf(in[r][f + c]);  swiglu: out = silu(in[r][c]) * in[r][f + c].  in bf16 [rows][ldi];
 *   f % 8 == 0, ldi >= 2 f, ldi % 8 == 0, ldo % 8 == 0, both pointers 16-byte aligned. */
int r3g_op_layernorm(const void* d_x, int x_format, int64_t ldx, int64_t x_batch_stride, uint16_t* d_y, int64_t ldy, int64_t y_batch_stride,
                     uint8_t* d_y8, int64_t ldy8, float* d_y_scale, const float* d_w, const float* d_b, const float* d_scale,
                     const float* d_shift, int64_t mod_stride, int seg2_row0, int seg2_row1, const float* d_scale2, const float* d_shift2,
                     int rows, int c, int rows_per_batch, float eps, void* stream);
int r3g_op_ln_dot(const void* d_x, int x_bf16, int64_t ldx, int rows, int c, int do_ln, const float* d_lnw, const float* d_lnb, float eps,
                  const float* d_w, float b, float* d_out, void* stream);
int r3g_op_qkv_split(const uint16_t* d_src, int64_t ld, int64_t src_batch_stride, int q_off, int k_off, int v_off, int head_stride,
                     uint16_t* d_q, uint16_t* d_k, uint16_t* d_vt, int lq_pad, int lk_pad, int dst_row0, int batch, int heads, int l,
                     int norm, const float* d_qw, const float* d_qb, const float* d_kw, const float* d_kb, float eps, float q_scale,
                     void* stream);
int r3g_op_group_norm(const float* d_x, int rows, int c, int groups, const float* d_gamma, const float* d_beta, float eps, int do_silu,
                      uint16_t* d_y, int nb, const float* d_addv, int64_t add_stride, void* stream);
int r3g_op_softmax_rows(const float* d_s, int64_t lds, uint16_t* d_p, int64_t ldp, int rows, int n, float scale, void* stream);
int r3g_op_geglu(const uint16_t* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int f, void* stream);
int r3g_op_swiglu(const uint16_t* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int f, void* stream);
/* The small kernels every sampling step and every staged input passes through, one launch each (csrc/elem.hip; vec_add:
 * csrc/conv_kernels.hip).  Test hooks (tests/test_vec_kernels_gpu.py).  The whole contract is checked in the entry point; a violation
 * is R3G_ERR_INVALID with nothing launched or written.  Common to all: every pointer named non-null unless stated, every size (b, k, n,
 * rows, c, count, njobs, s, ps) >= 1, a leading dimension at least the width.  All f32 unless stated.
 *
 * gemv: y [b][n] = act_out(act_in(x [b][k]) . w[row][:] + bias[row]), w bf16 [n][ldw], bias (may be null) [n]; act = SiLU where the
 *   flag is set.  1 <= b <= 8, k % 8 == 0, b * k * 4 <= 65536, ldw % 8 == 0, ldw >= k, w 16-byte aligned (16 bytes of w per lane).
 * gemv_multi: njobs matrices over ONE input, 1 <= b <= 2: job j writes y[out_off[j] + bi * n[j] + row] (no output activation).  w, bias
 *   (null, or an array whose entries may be null), ldw, n, out_off are HOST arrays of njobs entries, w[j] / bias[j] device pointers; per
 *   job the demands of gemv, and out_off[j] >= 0.  The entry point builds the device table itself and is synchronous.
 * timestep_embedding: out [b][256] = cos | sin (128 each) of t * time_factor * exp(-ln(10000) j / 128); d_t [b], or null: every row
 *   uses t_scalar.
 * fourier_grid: out bf16 [count][64] = rows start .. start + count - 1 of the dense lattice, point idx = (i (r + 1) + j) (r + 1) + k
 *   with coordinates np.linspace(-bound, bound, r + 1, dtype=float32); channels [x y z | sin(x_c 2^f [pi]), c major, f minor | cos
 *   likewise | zeros]; a row at or past (r + 1)^3 is the embedding of the origin.  r >= 1, start >= 0, 0 <= num_freqs, 3 + 6 num_freqs
 *   <= 64.
 * fourier_points: the same rows for listed points: row i < count is point d_list[i] (int32; bit for bit fourier_grid's row for that
 *   index), rows [count, rows) are the origin's.  1 <= count <= rows, out 16-byte aligned.  The list ENTRIES are the caller's
 *   responsibility (>= 0; an entry at or past (r + 1)^3 gives the origin's row): they are not read on the host.
 * cfg_euler: lat[i] += dsigma (vu + guidance (vc - vu)), vc = v2[i], vu = v2[n + i] (conditional half first), i < n.
 * euler_step: lat[i] += dsigma v[i]; float4 accesses when both pointers are 16-byte aligned, one element per lane otherwise.
 * nonfinite_flag: *d_flag |= 1 when x[0 .. n) holds a NaN or an infinity; never cleared.
 * cast_pad: out bf16 [rows][ldo]: out[r][col] = bf16(in[r][col] * scale) for col < c, 0 for c <= col < cpad; c <= cpad, ldi >= c, ldo >= cpad.
 * fill_rows: dst[r][col] = vals[col];  add_rows: x[r][col] += pos[r][col];  over [rows) x [c).
 * f32_to_bf16: out bf16 [n] = in [n], round to nearest even.
 * patch_rows: img [3][s][s] -> out bf16 [(s / ps)^2][kpad]: patch (py, px), column (ch ps + dy) ps + dx = img[ch][py ps + dy][px ps + dx],
 *   columns [3 ps^2, kpad) zero.  s % ps == 0, ps <= 1024, kpad >= 3 ps^2.
 * vec_add_inplace: y[i] += x[i];  vec_add: out[i] = a[i] + b[i], a null a or b standing for zeros (0.0f + b[i]);  i < n. */
int r3g_op_gemv(const float* d_x, int b, int k, const uint16_t* d_w, int64_t ldw, const float* d_bias, float* d_y, int n, int silu_in,
                int silu_out, void* stream);
int r3g_op_gemv_multi(const float* d_x, int b, int k, const void* const* w, const void* const* bias, const int64_t* ldw, const int* n,
                      const int64_t* out_off, int njobs, float* d_y, int silu_in, void* stream);
int r3g_op_timestep_embedding(const float* d_t, float t_scalar, int b, float time_factor, float* d_out, void* stream);
int r3g_op_fourier_grid(uint16_t* d_out, int64_t start, int count, int r, double bound, int num_freqs, int include_pi, void* stream);
int r3g_op_fourier_points(uint16_t* d_out, const int32_t* d_list, int count, int rows, int r, double bound, int num_freqs, int include_pi,
                          void* stream);
int r3g_op_cfg_euler(float* d_lat, const float* d_v2, int64_t n, float guidance, float dsigma, void* stream);
int r3g_op_euler_step(float* d_lat, const float* d_v, int64_t n, float dsigma, void* stream);
int r3g_op_nonfinite_flag(const float* d_x, int64_t n, int* d_flag, void* stream);
int r3g_op_cast_pad(const float* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int c, int cpad, float scale, void* stream);
int r3g_op_fill_rows(float* d_dst, int64_t ld, int rows, int c, const float* d_vals, void* stream);
int r3g_op_add_rows(float* d_x, int64_t ldx, const float* d_pos, int64_t ldp, int rows, int c, void* stream);
int r3g_op_f32_to_bf16(const float* d_in, uint16_t* d_out, int64_t n, void* stream);
int r3g_op_patch_rows(const float* d_img, int s, int ps, uint16_t* d_out, int kpad, void* stream);
int r3g_op_vec_add_inplace(float* d_y, const float* d_x, int n, void* stream);
int r3g_op_vec_add(const float* d_a, const float* d_b, float* d_out, int n, void* stream);
/* FP8 operands (BASELINE.json configs[3]).  Test / benchmark hooks; the model uses the same kernels for the geo decoder under
 * r3g_set_option("geo_fp8", 1).
 * quant_fp8: bf16 [rows][k] -> OCP e4m3 bytes [rows][k] + one fp32 scale per row; k % 8 == 0, ldx % 8 == 0, ldq % 8 == 0.
 *   scale = max(fl(amax fl(1 / 448)), 2^-126) for a row with amax > 0 and 1 for an all-zero row; code = the e4m3 nearest to
 *   fl(x fl(1 / scale)) (ties to even; the quotient exceeds 448 by three roundings at most and rounds to 448).  The floor -- the smallest normal fp32 -- keeps 1 / scale finite: a finite row never
 *   produces a NaN code, the decoded code times scale is within half an e4m3 step (2^-10 scale at least) of x, and only rows with
 *   amax < 448 * 2^-126 (about 5.3e-36) are touched by it.  The e4m3 output of r3g_op_layernorm scales its rows by the same rule.
 *   Non-finite elements are not repaired: a NaN element becomes the NaN code (0x7F under the sign bit) and does not enter amax, so the rest
 *   of its row is quantised as if it were absent; a +-Inf element makes the row's scale +Inf, its own code the NaN code and every finite
 *   element of the row a zero code (tests/test_fp8_edges_gpu.py pins both).
 * gemm_fp8: C = epilogue((scale_a[m] scale_w[n]) sum_k a8[m][k] w8[n][k] + bias) on v_mfma_scale_f32_16x16x128_f8f6f4 (twice the bf16
 *   matrix rate); epilogue 0, 1, 2 (bf16 out), 3 (fp32 residual), 6 (bf16 residual) as for r3g_op_gemm (gate null: 1); the GELU epilogues
 *   take their fp32 forms whatever "gelu_pk" says.  Any other epilogue is R3G_ERR_INVALID: 5 and 9-11 need operands this entry point
 *   cannot carry, 4 and 8 have no fp8 form, 7 is r3g_op_gemm_fp8_e4m3.  Shapes: m, n >= 0 (either 0: R3G_OK, nothing is launched),
 *   k >= 256, k % 256 == 0, n % 4 == 0.  Operands: a8 and w8 are staged 16 bytes at a time -- lda, ldw in bytes, % 16 == 0, both >= k,
 *   d_a8 and d_w8 16-byte aligned, m * lda and n * ldw below 2^32 (32-bit staging offsets); d_scale_a f32 [m] 4-byte aligned, d_scale_w
 *   f32 [n] 16-byte aligned (read four at a time); d_bias and d_gate (either may be null) 16-byte aligned, n floats each.  Output as for
 *   r3g_op_gemm: ldc % 4 == 0, ldc >= n, d_c aligned to four elements (8 bytes for 0, 1, 2, 6; 16 bytes for 3); with n % 8 == 0,
 *   ldc % 8 == 0 and a 16-byte aligned d_c the 16-bit outputs leave in 16-byte stores instead (same values).  Nothing outside [m) x [n)
 *   of C is written; rows past m / n and bytes past k of a8 and w8, and entries past m / n of the scales, bias and gate, are never read.
 *   A violation is R3G_ERR_INVALID with nothing launched or written.  Counter "gemm_fp8" moves by one per launch.
 * gemm_fp8_e4m3 (epilogue 7, the operand of a following fp8 GEMM under a static scale): c8[m][n] = the e4m3 code nearest to
 *   gelu_erf(lin) * fl(1 / out_scale) clamped to +-448 (fp32 GELU form, ties to even; a NaN stays the NaN code), lin as above; out_scale > 0 and finite.  The same contract
 *   with C in bytes: ldc_bytes % 4 == 0, ldc_bytes >= n, d_c8 4-byte aligned; with n % 16 == 0, ldc_bytes % 16 == 0 and a 16-byte aligned
 *   d_c8 the codes leave in 16-byte stores (same values). */
int r3g_op_quant_fp8(const uint16_t* d_x, int64_t ldx, int rows, int k, uint8_t* d_q, int64_t ldq, float* d_scale, void* stream);
int r3g_op_gemm_fp8(const uint8_t* d_a8, int64_t lda, const float* d_scale_a, const uint8_t* d_w8, int64_t ldw,
                    const float* d_scale_w, const float* d_bias, void* d_c, int64_t ldc, const float* d_gate, int m, int n,
                    int k, int epilogue, void* stream);
int r3g_op_gemm_fp8_e4m3(const uint8_t* d_a8, int64_t lda, const float* d_scale_a, const uint8_t* d_w8, int64_t ldw,
                         const float* d_scale_w, const float* d_bias, uint8_t* d_c8, int64_t ldc_bytes, float out_scale, int m, int n,
                         int k, void* stream);
/* Per-kernel-family timing with HIP events on the launch stream (bench.py's roofline leg).  Families, in order:
 * 0 gemm, 1 attention, 2 layernorm, 3 qkv_split, 4 gemv, 5 elementwise, 6 mc_classify, 7 mc_other, 8 mesh
 * cleaners (n >= 9).  work = algorithmic FLOPs (0,1,4) / bytes (6,8) summed over the launches since r3g_prof_enable(1). */
int r3g_prof_enable(int on);
int r3g_prof_read(int64_t* counts, double* ms, double* work, int n);
/* per family: algorithmic bytes (operands read once, result written once) of the launches whose `work` is FLOPs */
int r3g_prof_read_bytes(double* bytes, int n);
/* A/B switches for tests and ablations.  Default 1: "fuse_qkv" (QKV split/norm/transpose in the projection epilogue
 * vs a separate kernel), "batch_mods" (all adaLN modulations of a forward in one GEMV launch), "lds_dma"
 * (= r3g_set_staging), "cfg_dedup" (one weighted token for a uniform unconditional context), "group_streams" (img and
 * txt stream of a double block in one GEMM / LayerNorm launch), "geo_q_cache" (1: the part of the geo decoder that does not depend on the object -- Fourier features, query_proj, ln_1, c_q,
 * q-norm of every grid point -- stays resident in HBM after its first evaluation, 2 x 34.8 GB at 257^3, and is read instead of
 * recomputed; bit-identical; skipped by itself when the memory is not there), "skip_zero_step" (the DiT evaluation of a step with d_sigma = 0 --
 * upstream's last step -- is skipped: x += 0 * v), "overlap_mlp" (0 default | 1: MLP half of a single block's linear1
 * on a second stream beside the attention kernel), "gemm_wide_epilogue" (stores through the LDS transpose).  "lds_dma" 0 and "gemm_wide_epilogue" 0 keep every bit except (a) in
 * the geo decoder, whose folded epilogues ("geo_ln3_fold", "geo_lnd_fused") exist for LDS-DMA staging and the wide epilogue only:
 * without either it runs rounds 1-5's launches, as under "geo_ln3_fold" 0 + "geo_lnd_fused" 0; (b) "lds_dma" 0: the register-staged
 * attention kernel is the "attn_variant" 0 body, with that switch's corner; (c) "gemm_wide_epilogue" 0: the narrow fp32
 * read-modify-write epilogue forms old + gate (acc + bias) with one fused multiply-add where the wide one rounds the product first --
 * whatever runs on an fp32 residual stream (conditioner, VAE, the DiT's plain-batch forward) moves by an fp32 rounding per residual
 * GEMM, and stays at its tolerance against the fp32 oracle (tests/test_switches_gpu.py::test_switch[gemm_wide_epilogue=0]).
 * Tuning: "gemm_waves" (0 auto | 4 | 8 | 9 = 256x256 two-stage | 10 = 256x128 | 11 = 256x256 phased | 12 = phased,
 * persistent grid | 13 = phased, deterministic split-K over two workgroups per tile (another order of the fp32 additions, like "gemm_splitk") | 16 | 32 = deep ring), "gemm_raster" (-1 auto | tile columns per rasterisation group), "gemm_phased"
 * (1: 256x256 tiles on the phased counted-vmcnt kernel), "gemm_persistent" (1: its persistent form for bf16 outputs
 * with more tiles than CUs), "gemm_xcd_walk" (1 default: in the persistent form an XCD's workgroups walk ONE contiguous range of the
 * rasterised tile order (consecutive steps touch neighbouring A rows) -- geo c_fc 1 109 -> 1 045 us, L2 <-> fabric bytes unchanged; bit-identical | 0: rounds 2-4's walk), "gemm_persistent_resid" (0 | bit 0: the fp32, bit 1: the bf16 read-modify-write epilogue on the persistent form as well), "gemm_num_cu" (CUs the tile rules assume, default 256), "gemm_auto_rule" (2: the current
 * tile-choice rule | 1: round 2's | 0: round 1's first version), "attn_generation" (7 default: 6 where its
 * 256-query workgroups make four rounds of the device, otherwise 2 | 2 = four waves of 32 queries | 6 = four waves of 64
 * queries, bit-identical to 2 | 1 = the first-round kernel | 3, 4, 5 = pipelined / 8-wave variants), "attn_wide_min" (2048: work items of 256 queries from which attn_generation 7 takes generation 6; while "attn_interleave" is automatic and "attn_variant" 1, ragged launches -- the DiT's joint attention -- take it from 1024 on whatever this value, because the skewed body makes it the faster kernel there; such a launch votes on its safe pass per 128 queries as generation 2 does and keeps generation 2's bits, profiles/attention_skew.md), "ln_rows" (0 automatic | 1 | 4 rows per wave in the
 * LayerNorm / ln_dot row kernels), "ln_rows4_min" (65536: launches of at least this many rows take 4 rows per wave under the automatic rule), "ln_fixed" (1: their instantiations with a compile-time row length for C = 1024 / 1536), "ln_modes" (1, round 6: for C = 1024 the affine-only and the modulation-only launches take instantiations with that decided at compile time -- bit-identical | 0: the generic kernel), "attn_pipelined" (0 default | 1: the software-pipelined form of the first-round kernel, other rounding points inside the softmax like
 * attn_generation 1), "attn_ablate"
 * (timing-only masks, results are garbage), "floater_by_vertex" (0), "mc_rows" (4 | 8 | 16 | 32 node rows per wave in the marching-cubes row
 * kernel), "mc_deferred" (1: tiling selection batched per wave | 0: round 1's per-row kernel), "geo_resid_bf16" (1:
 * 16-bit residual stream in the geo decoder block | 0: round 1's fp32 stream, without the query-side cache and the folded epilogues --
 * another precision of the stream, NOT bit-preserving), "geo_fp8" (0 default | 1: the geo decoder's c_q and MLP GEMMs on e4m3
 * operands | 2: MLP only | 3: c_q only -- a different precision, NOT result-preserving), "gemm_splitk" (0 default | 1: an under-filled deep-K fp32-residual GEMM splits K over two workgroups per 256x256 tile -- another order of
 * the fp32 additions, not bit-preserving; deterministic), "conv_implicit" (1 default: the 3 x 3 convolutions of the texture models run as implicit GEMMs -- the 128 x 128
 * kernel gathers the nine shifted rows of its A operand from the activation rows itself, bit-identical to the GEMM over the im2col
 * matrix | 0: im2col + GEMM, rounds 3-4), "gemm_splitk128" (1 default: the 3 x 3 convolutions of the texture models split a deep k over
 * several workgroups where their grid would fill less than half of the chip, r3g_op_gemm_splitk | 0: one workgroup per tile walks all of k, rounds 2-4 -- another
 * order of the fp32 additions, not bit-preserving), "geo_q_cache_gb" (the
 * budget of geo_q_cache in GiB; < 0, the default: 30 % of the device's memory; a grid that needs more gets a prefix of its passes
 * cached), "dit_resid_f16" (1 default: the residual stream of the DiT's de-duplicated CFG path in fp16 -- the reference's own
 * activation type -- | 0: in fp32, rounds 1-3; NOT bit-preserving: 50-step latents at full depth 3.3e-3 against 3.0e-3 from the
 * fp32 oracle, tests/test_cfg1_golden_gpu.py; -21 ms per object), "gelu_pk" (1 default: the GELU epilogues of the GEMMs evaluate x S(x) with S in packed fp16 -- csrc/gemm_common.h: a
 * degree-6 polynomial on v_pk_fma_f16, |error of S| <= 7.5e-4 as evaluated in fp16 (6.5e-4 tanh / 7.2e-4 erf measured; the fit alone 1.2e-4), +1.2 % on the rel-L2 error behind the bf16 rounding of the output |
 * 0: rounds 3-4's fp32 forms with v_exp_f32 / v_rcp_f32; NOT bit-preserving), attn_generation 9 (opt-in, round 5: the phased 12-wave kernel -- three groups of four
 * waves one phase apart, a wave's matrix phase under the two softmax phases of its SIMD neighbours; bit-identical to generations 2
 * and 6, measured slower: profiles/r05_attention_phases.md), "attn_prio" (generation 9: 0 no s_setprio | 1 its matrix phase at priority 1 | 2 its softmax phases), "attn_stamps" (0 | 1: attn_generation 9 prints the s_memtime ticks of its
 * phases, work and barrier wait, per launch to stderr -- timing experiments, synchronous), "dit_f16_guard" (1 default: the final latents of a launch group that ran
 * on the fp16 stream are checked for NaN / infinity and a group that overflowed runs again on the fp32 stream, with a line on
 * stderr | 0: no check),
 * "attn_variant" (round 6; generations 2 / 6 / 7: 1 default -- the FAST pass takes no maximum after the first key block and tests
 * the sum of a lane's 16 exponentials against 2^16 into a sticky flag; a workgroup whose valid queries set it runs its query tile
 * again with variant 0's body | 0 = rounds 2-5.  Bit-identical to variant 0 unless variant 0 would have moved its stabiliser where
 * the fast pass does not: then equal within the bf16 rounding of P),
 * "attn_interleave" (where "attn_variant" 1 runs the 64-query-per-wave kernel, the order in which the unmasked key blocks of its fast
 * pass issue their softmax; every value computes the same bits.  0 default: automatic -- the form the pipeline A/B of
 * profiles/attention_skew.md found faster for the launch's class: the skewed one (value 2) for launches of at least 2048 work items
 * of 256 queries and ragged launches of at least 1024, the clustered one (value 3) for the rest | 1: the softmax of one
 * score block between the MFMAs of another INSIDE a key tile, measured 2-3 % slower, profiles/attention_interleave.md | 2: the same
 * skew ACROSS key blocks in steady state, every MFMA gap filled, the K half of the staging ring one tile ahead of the V^T half,
 * profiles/attention_skew.md | 3: clustered, the softmax behind the score MFMAs; other values are ignored),
 * "attn_async_stage" (1 default | 0: the "attn_variant" 1 kernels issue the LDS-DMA of the next K / V^T tile through the compiler's
 * builtin, which makes it wait for the transfer in front of the current tile's first fragment read instead of at the tile's end;
 * bit-identical either way, profiles/attention_interleave.md),
 * "geo_ln3_fold" (1 default, round 6 | 0: the geo decoder's ln_3 as its own launch writing a normalised bf16 copy of the stream, rounds
 * 1-5; folded, c_proj's epilogue also writes the rows' chunk statistics, and c_fc runs on the raw stream with W' = bf16(W gamma) and
 * rstd (acc - mean c1) + c2 in front of its GELU -- the same function without the bf16 rounding of the normalised operand: logits move
 * by 4-6e-3 of their scale (recorded in tests/test_model_gpu.py), inside the 1e-2 tolerance against the fp32 oracle; taken only where the GEMM
 * launcher serves the folded epilogues -- LDS-DMA staging and "gemm_wide_epilogue" on -- otherwise rounds 1-5's launches run),
 * "geo_lnd_fused" (1 default, round 6 | 0: the geo decoder's ln_post + output_proj as their own launch over the stored residual
 * stream, rounds 1-5; fused, the last residual GEMM's epilogue writes per-row statistics of its 64-column chunks instead of the
 * stream and a small kernel merges them -- same function, another summation order: logits equal to ~1e-6 of their scale; under the
 * same condition as "geo_ln3_fold"),
 * "gemm_epi_slices" (1 default, round 6 | 0: the persistent phased kernel's bf16 / fused-QKV epilogues in 32-row passes through 4 KiB of
 * extra scratch per wave instead of 64-row passes through the wave's own staging slices of the idle k-tile buffer), "gemm_mixed" (1
 * default, round 6 | 0: a DiT single block's fused QKV projection and MLP-in + GELU projection as two launches instead of one
 * persistent launch over both problems' tiles), "gemm_persistent_qkv" (1 default since round 6 | 0: fused QKV launches with more 256x256 tiles than CUs -- the double
 * blocks' img + txt pair, and the single blocks' QKV half, which then leaves the "gemm_mixed" launch -- one tile per workgroup instead of the
 * persistent phased kernel; with round 4's 32-row epilogue passes the
 * persistent form was 17 ms per object slower, with "gemm_epi_slices" it is 4 ms faster, profiles/r06_ab.md), "flow_first_step" / "flow_last_step" (0 / -1: r3g_flow_sample runs steps [first, last) of its schedule; consecutive
 * segments continuing on each other's latents are the same launches as one call -- how tests read the latents after 10, 20, ...
 * of 50 steps), "geo_kv_topk" / "geo_kv_group" / "geo_kv_stride" (0 / 8192 / 64: adaptive top-k KV selection in the geo decoder,
 * described above r3g_kv_selection_last; values outside their ranges are refused), "geo_narrow_fused" (0 default; only a
 * narrow geo decoder of width 256 with hidden 256 | 512 | 1024 on the bf16 stream is affected -- 1: everything behind its
 * cross-attention, c_proj to output_proj, is one launch per pass (r3g_op_geo_tail's kernel) | 0: the generic launches; the same
 * function with other rounding points; profiles/turbo_vae.md has the timing).  None of them changes a
 * result bit, except fuse_qkv / batch_mods / cfg_dedup (different summation order, same function), attn_generation and
 * attn_pipelined (different rounding points inside the softmax), and those whose description above says so: geo_fp8, geo_resid_bf16,
 * dit_resid_f16, gelu_pk, gemm_splitk, gemm_waves 13, gemm_splitk128, geo_ln3_fold, geo_lnd_fused, geo_narrow_fused, attn_variant in its stated
 * corner, and lds_dma / gemm_wide_epilogue where their description says so.  r3g_get_option reads every one of them back. */
int r3g_set_option(const char* name, int value);
/* The current value of every name r3g_set_option accepts (the "geo_kv_*" names and "geo_narrow_fused" included), as r3g_set_option
 * would take it back: "geo_q_cache_gb" reports -1 for the automatic budget, "flow_last_step" -1 for "to the end", "lds_dma" 1 only
 * while both the GEMM and the attention kernels stage through LDS-DMA.  A value that r3g_set_option clamped or refused reads back as
 * what is in force.  Host state only (no GPU needed).  Unknown name: R3G_ERR_INVALID. */
int r3g_get_option(const char* name, int* value);
/* The names r3g_set_option accepts, one per index from 0 on, in no particular order; NULL for an index below 0 or past the last name. */
const char* r3g_option_name(int index);
/* Process-wide event counters (round 6).  "dit_f16_fallbacks": launch groups of r3g_flow_sample_batch whose fp16 residual stream
 * produced non-finite latents and that therefore ran a second time on the fp32 stream ("dit_f16_guard"; such a group costs twice its
 * time -- bench.py and the stage report carry the count so that a slow run says why).  "dit_groups": launch groups run so far.
 * "dit_evals": DiT evaluations issued so far, one per launch group and evaluated step (49 for upstream's 50-step schedule, whose
 * last step is skipped; N for an N-step consistency table; an fp32 re-run counts again).
 * "geo_q_cache_builds": allocations of the geo decoder's query-side cache so far (a change of (R, bound) frees and allocates it
 * again; r3g_grid_query_points and the coarse levels of r3g_grid_query_hier never do).
 * "geo_kv_groups": (group, head) selections of top-k KV selection so far.
 * "geo_narrow_passes": grid passes served by the fused tail of a narrow geo decoder ("geo_narrow_fused") so far.
 * "meshdist_tests": point-triangle tests made by r3g_meshdist_query, and by the walks of r3g_meshfit_step / r3g_meshfit, so far.
 * "meshinside_tests": point-face tests made by r3g_meshinside_query so far.
 * "meshfit_steps": accumulation launches of the mesh registration (r3g_meshfit_step, and each one r3g_meshfit makes) so far.
 * "meshtopo_builds": successful builds of the mesh topology (r3g_meshtopo_build, and the one or two r3g_meshtopo_orient makes) so far.
 * "meshtopo_rounds": label rounds those builds launched so far.
 * "meshfill_plans": successful plans of the mesh fill (r3g_meshfill_plan) so far.
 * "meshfill_rounds": pointer-doubling rounds those plans launched so far (twice the report's `rounds` each).
 * "cloud_tests": point-point distance tests made by r3g_cloud_knn so far.
 * "orient_rounds": Boruvka rounds launched by r3g_cloud_orient so far.
 * "dbscan_launches": kernels launched by r3g_cloud_dbscan so far (per call: a number that does not depend on the data).
 * "dbscan_tests": evaluations of the neighbour predicate made by r3g_cloud_dbscan so far.
 * "recon_solves": successful r3g_recon_solve calls so far; "recon_cycles": the V-cycles they ran.
 * "device_bytes_live": bytes of device memory the library holds right now, over all contexts of the process: every buffer it keeps
 *   between calls (workspaces, the model and UNet arenas, the geo decoder's query-side cache, the DiT batch arena; not pinned host
 *   buffers, not torch's allocator).  A gauge, not an event count: r3g_destroy and r3g_model_trim bring it down.
 * "geo_lnf_passes" / "geo_lnd_passes": geo decoder passes that took the folded ln_3 ("geo_ln3_fold") / ln_post + output_proj
 * ("geo_lnd_fused") epilogues.
 * Kernel-choice counters, one per form a launch can end in, bumped on the host where the launch is issued (tests read them to see
 * that a switch was obeyed, the forms being bit-identical more often than not).  GEMM: "gemm_w4_128", "gemm_w8_128" (128 x 128 tiles,
 * 4 | 8 waves), "gemm_w16_256" (256 x 256, 16 waves), "gemm_two_stage_256" ("gemm_waves" 9), "gemm_256x128" (10), "gemm_phased" (one
 * tile per workgroup; the folded geo epilogues included), "gemm_phased_persistent", "gemm_mixed" (a single block's fused QKV + MLP-in
 * as one persistent launch), "gemm_splitk2" (split-K over two workgroups per tile), "gemm_splitk128" (the slices of the 128 x 128
 * kernel plus their reduce; the slice launch counts under its own form as well), "gemm_deep_ring", "gemm_conv_implicit",
 * "gemm_register_staged" (a tile-kernel launch without LDS-DMA; the phased kernels have no such form), "gemm_fp8" (the e4m3-operand form
 * of the phased kernel: r3g_op_gemm_fp8, r3g_op_gemm_fp8_e4m3 and the geo decoder under "geo_fp8"; no other GEMM counter moves with it).  Attention: "attn_gen1",
 * "attn_pipelined", "attn_gen2", "attn_gen3", "attn_gen4", "attn_gen5", "attn_gen6", "attn_gen9" (the generation launched, after "attn_generation" 7's rule), and
 * "attn_register_staged".  Row kernels: "ln_rows1" / "ln_rows4" (LayerNorm and ln_dot launches with 1 | 4 rows per wave), "ln_fixed_count"
 * (with a compile-time row length), "ln_mode_inst" (with the affine-only / modulation-only instantiation); "mc_rows4", "mc_rows8",
 * "mc_rows16", "mc_rows32" (marching-cubes row-kernel classify launches by node rows per wave) and "mc_deferred_rows" (those with the
 * deferred tiling selection).  All counters are atomic: two contexts on two threads may bump them concurrently.
 * r3g_flow_sample_batch is SYNCHRONOUS while the guard is on (one 4-byte read-back per group) and must not be captured into a
 * hipGraph then; with "dit_f16_guard" 0 or "dit_resid_f16" 0 it only enqueues work.  Unknown name: R3G_ERR_INVALID. */
int r3g_get_counter(const char* name, int64_t* value);
/* The names r3g_get_counter accepts ("device_bytes_live" included), enumerated like r3g_option_name: NULL outside [0, count). */
const char* r3g_counter_name(int index);
/* operand staging of the MFMA kernels: 1 = LDS-DMA (global_load_lds, default), 0 = through registers */
int r3g_set_staging(int use_lds_dma);

#ifdef __cplusplus
}
#endif
#endif
