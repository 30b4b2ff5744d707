/*
 * tsl_hip.h -- C ABI of libtsl_hip.so, the MI355X (gfx950) thin-shell engine.
 *
 * Drop-in boundary.  The reference (Genesis-Embodied-AI/ThinShellLab) has no FFI layer: its engine
 * is a set of Python objects (code/engine/BaseScene.py, model_fold_offset.py, ...) whose methods the
 * task scenes / Grad / trajopt scripts call.  This header declares what a Python `engine` package binds
 * with ctypes so that those callers keep working; every entry point names the reference method it
 * replaces (file:line under /root/reference/code).  See INTEGRATION.md for the binding stub.
 *
 * Conventions: extern "C"; plain pointers and sizes; all reals fp64 and all indices int32 like the
 * reference (ti.init(default_fp=ti.f64, default_ip=ti.i32)); return 0 on success, <0 on error
 * (message via tsl_last_error()).  Pointers named *_dev are device (HBM) pointers owned by the caller
 * (torch tensors); pointers named *_host are host memory.  No ownership is transferred.  The library
 * owns only the opaque tsl_ctx (topology, system matrix, scratch).  Work is enqueued on the stream set
 * with tsl_set_stream(); calls that return a host scalar synchronise that stream.
 * One context per GPU / per scene; contexts are independent (one process per GPU, no collectives).
 */
#ifndef TSL_HIP_H
#define TSL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsl_ctx tsl_ctx;

/* One cloth (engine/model_fold_offset.py:10-107).  Index tables are the ones Cloth.init_mesh builds
 * (model_fold_offset.py:928-1018), LOCAL vertex / face numbering; v_offset = Cloth.offset. */
typedef struct {
  int32_t N, M, NV, NF, v_offset;
  double dx, mass, Kl, Ka, Kb, k_angle;
  const int32_t* f2v_host;           /* NF x 3 */
  const int32_t* counter_face_host;  /* NF x 3 */
  const int32_t* counter_point_host; /* NF x 3 */
  const double* rest_area_host;      /* NF      Cloth.V   (model_fold_offset.py:835) */
  const double* rest_len_host;       /* NF x 3  Cloth.l_i (model_fold_offset.py:836-838) */
} tsl_cloth_desc;

/* One tetrahedral body.  kind 0: engine/model_elastic_tactile.py (stable Neo-Hookean, alpha);
 * kind 1: engine/model_elastic_offset.py (Neo-Hookean with log J).  B = F_B (Ds^-1), W = F_W. */
typedef struct {
  int32_t kind, n_verts, n_cells, v_offset;
  double mu, lam, alpha;
  const int32_t* tets_host; /* n_cells x 4, LOCAL vertex ids */
  const double* B_host;     /* n_cells x 9 row-major */
  const double* W_host;     /* n_cells */
} tsl_elastic_desc;

/* One BaseScene.contact_pair_analysis call of the scene's contact_analysis()
 * (BaseScene.py:818-835, Scene_folding.py:99-108): query vertices [v_start, v_end) against body b_idx. */
typedef struct {
  int32_t b_idx, v_start, v_end;
  int32_t mu_is_param; /* 0: use mu; 1 / 2: the live mu_cloth_elastic / mu_cloth_cloth parameter (times mu when mu > 0) */
  double mu;
} tsl_contact_pair;

/* Body ranges of BaseScene.body_list (BaseScene.py:91-99). */
typedef struct { int32_t v_start, v_end, f_start, f_end; } tsl_body;

typedef struct {
  int32_t tot_NV, tot_NF;
  double dt, k_contact, eps_contact, eps_v, damping; /* BaseScene.py:44-48, scene init_scene_parameters */
  int32_t max_n_constraints;
  int32_t n_cloth;   const tsl_cloth_desc* cloths;
  int32_t n_elastic; const tsl_elastic_desc* elastics;
  int32_t n_body;    const tsl_body* bodies;
  int32_t n_pair;    const tsl_contact_pair* pairs;
  const double* mass_host;      /* tot_NV      BaseScene.mass (BaseScene.py:332-346) */
  const double* gravity_host;   /* tot_NV x 3  per-vertex gravity acceleration of its body (BaseScene.py:361-379) */
  const int32_t* faces_host;    /* tot_NF x 3  BaseScene.faces, GLOBAL vertex ids (BaseScene.py:348-359) */
  const int32_t* frozen_host;   /* 3*tot_NV    BaseScene.frozen (BaseScene.py:80, set_frozen) */
  double grid_h;                /* geometry.py:8 (0.003) */
} tsl_scene_desc;

typedef struct {
  int32_t newton_iters, ls_evals, cg_iters, solves, restarts, fallback, nc;
  double last_delta, last_alpha, energy;
  /* convergence accounting of the step's linear solves (the reference's spsolve is exact every time, sparse_solver.py:85-105):
   * fallback = solves that needed a second solver and converged there (flag 1); unconverged = solves that ended with flag 3;
   * attained = solves accepted by the attainable-accuracy rule (iterative solvers: true residual stagnating within 100x of cg_tol;
   * direct path: stagnating with a normwise backward error <= 1e-12, what a backward-stable direct solver delivers);
   * factorizations = numeric factorisations of the direct preconditioner; max_rel_residual over the step's solves */
  int32_t unconverged, attained, factorizations, plans;
  double max_rel_residual, max_backward_error;
} tsl_step_stats;

typedef struct {
  int32_t iters, restarts, flag; /* flag 0 converged with the primary solver, 1 converged with a fallback solver, 3 NOT converged */
  double rel_residual;           /* true residual |b - Hx| / |b| of the returned solution */
  int32_t method;                /* solver that produced x: 0 PCG, 1 MINRES, 2 GMRES, 3 BiCGStab, 4 sparse LU + iterative refinement (GMRES where that stalls) */
  int32_t attained;              /* 1: accepted by the attainable-accuracy rule instead of rel_residual <= cg_tol */
  double backward_error;         /* method 4: |b - Hx| / (|H|_inf |x| + |b|) of the returned solution (0 if not evaluated); |H|_inf is the norm
                                    of the static part only (the contact blocks are left out: the value can only overstate the error) */
} tsl_solve_stats;

const char* tsl_version(void);
const char* tsl_last_error(void);

/* BaseScene.__init__ + init_objects + init_property + set_frozen: upload topology, build the BSR(3x3)
 * pattern (replaces SparseMatrix's dense n x n storage, sparse_solver.py:13-17). */
int tsl_ctx_create(const tsl_scene_desc* desc, tsl_ctx** out);
void tsl_ctx_destroy(tsl_ctx* ctx);
int tsl_set_stream(tsl_ctx* ctx, void* hip_stream);

/* 0-d field writes of the reference and the engine's own switches (49 keys + three patterns; an unknown key is an error).
 *  Scene (trajopt_folding.py:50,66; Scene_folding.py:30-31; geometry.py:8-19; geometry_self.py:166-230):
 *   "cloth<i>.Kb|Kl|Ka|k_angle", "elastic<i>.mu|lam|alpha", "mu_cloth_elastic", "mu_cloth_cloth", "k_contact", "eps_contact", "eps_v", "damping",
 *   "k_handle" (0 default: stiffness in N/m of the soft handles of tsl_set_handles; negative fails; with 0, or with no handles, no handle kernel is launched),
 *   "k_tie" (0 default: stiffness in N/m of the ties of tsl_set_ties; negative fails; with 0, or with no ties, no tie slot exists and no tie kernel is launched),
 *   "k_collider" (0 default: stiffness in N/m shared by the half-space colliders of tsl_set_colliders; negative or non-finite fails; with 0, or with no
 *   colliders, no collider kernel is launched),
 *   "k_sphere" (0 default: stiffness in N/m shared by the sphere colliders of tsl_set_spheres; negative or non-finite fails; with 0, or with no
 *   spheres, no sphere kernel is launched),
 *   "k_capsule" (0 default: stiffness in N/m shared by the capsule colliders of tsl_set_capsules; negative or non-finite fails; with 0, or with no
 *   capsules, no capsule kernel is launched),
 *   "k_box" (0 default: stiffness in N/m shared by the rounded-box colliders of tsl_set_boxes; negative or non-finite fails; with 0, or with no
 *   boxes, no box kernel is launched),
 *   "k_sdf" (0 default: stiffness in N/m shared by the sampled distance-field colliders of tsl_set_sdfs; negative or non-finite fails; with 0, or
 *   with no fields, no field kernel is launched),
 *   "cloth<i>.membrane" (0 default: edge springs Kl + area term Ka, as the reference; 1: a St. Venant-Kirchhoff membrane per face, A0 Psi(F) with
 *   F = [x1 - x0, x2 - x0] Dm^-1, Dm the rest triangle rebuilt from the face's rest lengths (fails naming a face whose lengths violate the triangle
 *   inequality), Psi = mu |E|^2 + lam/2 tr(E)^2, E = (F^T F - I) / 2, A0 the rest area; it replaces the springs and the area term of the cloth's
 *   faces, bending / inertia / contact unchanged; spd 1 clamps the 6 x 6 d2Psi/dF2 by eigen-clamp, "spd_literal" does not apply to it; any value but
 *   0 / 1 fails), "wind_cn", "wind_ct" (0 default: the normal and the tangential drag coefficient in N s / m^3 of the wind of tsl_set_wind; negative or
 *   non-finite fails; with both 0, or with no wind list, no wind kernel is launched), "cloth<i>.stvk_mu", "cloth<i>.stvk_lam" (its Lame parameters in N/m, default 0; Kl / Ka of a StVK cloth are kept unused, as are
 *   stvk_* of a spring cloth; switching at any time keeps the block pattern and the plans of the factorisation),
 *   "newton_cap", "plastic", "contact" (0: no detection in tsl_step), "grid_h", "grid_extent" (broad-phase cell and box), "self_contact<body>"
 *   (0 / 1: the body's vertices are also projected onto its own triangles), "contact_ee" (0 default: vertex-triangle contact only, as the reference;
 *   1: edge-edge constraints between the surface edges of different bodies are appended behind the vertex-triangle ones, see tsl_contact_counts), "adj_clamp", "adj_clamp_angleref" (the clamping of analytic_grad_single:
 *   1000, on; of analytic_grad_system: 1, off), "adj_spd_pc" (adjoint solves of the iterative hierarchy preconditioned from the projected assembly).
 *  Linear solve (no reference counterpart: the reference calls cupyx spsolve):
 *   "cg_tol" (1e-10), "cg_maxit", "direct" (-1 auto: cloth grids of >= 1024 cells / 0 iterative hierarchy only / 1 always: multifrontal LU on the GPU),
 *   "direct_leaf" (vertices per nested-dissection leaf, 64), "direct_piv_tol" (static pivoting: pivots below this fraction of their entry diagonal are
 *   perturbed to it, 1e-11), "direct_berr" (1e-12: a first pass of the factorised solve whose normwise backward error |b - Hx| / (|H|_inf |x| + |b|) is
 *   at most this is accepted; 0: every solve is refined to cg_tol), and whose forward residual is at most 50 x cg_tol (fixed),
 *   "direct_flow" (3; bit 0: the block steps of one batch per tree level as ONE persistent dataflow launch, k_ds_gj_flow; bit 1: also the batches the
 *   LDS kernel would take; 0: one launch per 32 pivots -- the same bits either way), "direct_flow_token" (0: hand the device's dataflow token back),
 *   "direct_small_rounds" (2: rounds of the chip a batch may take in the LDS kernel k_ds_inv_small), "direct_g32_below" (1100: G = W F12 of a batch
 *   with fewer 64 x 64 tiles than this uses 32 x 32 tiles), "direct_gemv_wide_below" (300: a sweep launch of fewer 16-row chunks than this runs four
 *   workgroups per chunk), "direct_lookahead" (103; bit 0: on the tree levels of one batch each the leading block of every Schur complement is formed first and
 *   the parents' pivot blocks are gathered and inverted next to the rest of the Schur launch on a low-priority second stream; bit 1: the upward sweep of the solve's
 *   first application runs on that stream next to the chains of the last three levels -- levels [0, c0) next to the third from the top, [c0, c1) next to the one below the
 *   root, [c1, root) next to the root's, c0 = (value >> 2) & 7, c1 = (value >> 5) & 15 (0: none next to the root's); 0: one after the other -- the same bits).
 *   (Fixed since round 6: batches of >= 64 fronts launch their GEMM tiles with the XCD-aware map, the leaf panels of the next
 *   factorisation are cleared on a side stream after each solve of a time step, 64 plans of earlier constraint sets are kept.)
 *   "mg" (-1 auto / 0 / 1), "mg_coarse_exact", "mg_dense_nodes" (largest multigrid level solved exactly; -1 = chosen per time step), "body_inv"
 *   (dense inverses of the small FEM-body blocks), "gmres_m" (GMRES restart length), "tet_warm" (1: the eigen-clamp of the element blocks starts from
 *   the eigenvectors of the element's previous assembly), "spd_literal" (0 default: the forward projections of the cloth spring blocks, the contact normal
 *   blocks and the tactile element blocks are a converged Jacobi eigen-clamp; 1: the reference's own projector, SPD_Projector of linalg.py:15-148 --
 *   Householder, at most K = 10 (3 x 3) / 20 (9 x 9) shifted-QR sweeps, rebuild from the positive diagonal -- with the reference's arithmetic: the
 *   same bits as its x86-64 restatement in oracle/tslo_linalg.h for the same block.  The preconditioner-only assembly and the adjoint are not affected).
 *   (Element gradients / blocks and contact rows go to staging slots and records and are summed by gather kernels in a fixed order, constraint lists are
 *   compacted by scan, energies and dot products joined from per-workgroup partials: no f64 atomics on the step and adjoint path, two runs give the same
 *   bits.  There is no switch: the scattered-atomics assembly of rounds 1-3 and its "deterministic" key are gone.)
 *  Diagnostics: "verbose" (1 phase times per step, 2 plans, 3 batches, 4 Newton iterations, 5 refinement passes), "ds_dbg" (21 / 22: force the dataflow-abort
 *   branch, tests -- 22 with the rule that a first loss takes only the look-ahead away; 30: device-clock trace of a dataflow chain), "ds_bench_batch" (tsl_bench_direct on one batch).
 * The experiment switches of rounds 1-4 (factor lagging, alternative GEMM / Schur tilings, one-lane contact and 16-lane element assembly, PCG warm
 * start, ...) are gone with the code they selected; the measurements that retired them are in profiles/README.md and DESIGN.md section 9. */
int tsl_set_param(tsl_ctx* ctx, const char* key, double value);
int tsl_set_frozen(tsl_ctx* ctx, const int32_t* frozen_host);          /* BaseScene.set_frozen */
int tsl_set_ext_force(tsl_ctx* ctx, const double* ext_force_host);      /* BaseScene.ext_force / manipulate_force */
int tsl_set_gravity(tsl_ctx* ctx, const double* gravity_host);          /* per-vertex, tot_NV x 3 */

/* Soft handles (no reference counterpart: its only hold on a vertex is set_frozen): handle i is a spring from vertex verts[i] to a world-space
 * target t_i, E_h = 1/2 k_handle sum_i w_i |x_{v_i} - t_i|^2 with the scalar "k_handle" of tsl_set_param.  The term enters tsl_energy,
 * tsl_assemble (gradient row v_i: k_handle w_i (x - t_i); diagonal block: k_handle w_i I_3, positive semi-definite as it stands, so every spd mode
 * and "spd_literal" add the same numbers), tsl_step, tsl_adjoint_step and both scene-group steps; frozen dofs follow the mask rule of every other
 * term.  The block pattern, the plans of the factorisation and their cache do not depend on handles.
 * Conventions of tsl_set_ext_force: host pointers, the stream is synchronised, the lists are copied into buffers of the context.
 *   tsl_set_handles: n handles (global vertex ids); weights_host == NULL: every weight is 1; n = 0 removes all handles (the launches of a context
 *     that never had any).  Fails, naming the offender, for a vertex out of range, a vertex with more than one handle, a negative or non-finite
 *     weight.  The targets start at zero: set them before use.
 *   tsl_set_handle_targets: n x 3, the targets of the next energy, assemble, step or adjoint step.  The adjoint re-assembles the operator at x_s;
 *     tsl_handle_grad and the "k_handle" key of tsl_param_grad_keys read the targets: set the targets of step s before the reverse step s.
 *   tsl_handle_force: out_host (n x 3) = k_handle w_i (t_i - x_{v_i}), the force handle i applies to the cloth; frozen dofs are NOT masked
 *     (a read-out, like tsl_elastic_force).
 *   tsl_handle_grad: the contribution of one reverse step to d(loss)/d(t_i), sign of tsl_param_grad_keys: out_host (n x 3) = -p . dF/dt_i =
 *     k_handle w_i p_{v_i} on free dofs, exactly 0 on frozen ones; p_dev == NULL: the solution of the last tsl_adjoint_step. */
int tsl_set_handles(tsl_ctx* ctx, const int32_t* verts_host, const double* weights_host, int32_t n);
int tsl_set_handle_targets(tsl_ctx* ctx, const double* targets_host);
int tsl_handle_force(tsl_ctx* ctx, const double* pos_dev, double* out_host);
int tsl_handle_grad(tsl_ctx* ctx, const double* p_dev, double* out_host);

/* Soft handles at barycentric points of faces (no reference counterpart): handle i sits on face faces[i] = (v_0, v_1, v_2) of the scene's global face
 * table (tsl_scene_desc.faces_host: a cloth face or a surface face of a FEM body) with barycentric coordinates b_i and pulls the point
 * p_i = sum_a b_a x_{v_a} to its target, E_h = 1/2 k_handle sum_i w_i |p_i - t_i|^2: gradient row v_a: k_handle w_i b_a (p_i - t_i), block (v_a, v_b):
 * k_handle w_i b_a b_b I_3 -- an outer product times I_3, positive semi-definite as it stands, so every spd mode and "spd_literal" add the same
 * numbers.  Any number of handles may share a face or a vertex; b = (1, 0, 0) is a vertex handle without the one-per-vertex limit.  The nine blocks
 * of a face exist in the pattern: the plans of the factorisation and their cache do not depend on the handles.  Frozen dofs follow the mask rule.
 * One lane per touched vertex (gradient) and per touched block (matrix) adds its entries in a fixed order and writes once: no atomics, the same bits
 * run to run.  Conventions of tsl_set_handles.
 *   tsl_set_handles_on_faces: REPLACES the handle list, as tsl_set_handles does: a context holds a vertex list or a face list, either setter drops the
 *     other kind's list and all frames, and the targets start at zero.  bary_host: n x 3, used as given (not renormalised); weights_host == NULL:
 *     every weight is 1; n = 0 removes the handles.  Fails, naming the offender, and leaves the previous list in place for a face outside
 *     [0, tot_NF), a coordinate that is not finite or outside [0, 1], a triple whose sum differs from 1 by more than 1e-9, a negative or non-finite
 *     weight, a pair of the face's vertices without a block in the pattern (cannot happen for a scene's own faces).
 *   tsl_handle_points: out_host (n x 3) = the points p_i at the state pos; for a vertex list x_{v_i}.
 *   Every other handle and frame entry point works on a face list by handle index: tsl_set_handle_targets, tsl_handle_targets, tsl_handle_force
 *     (k_handle w_i (t_i - p_i), not masked), tsl_handle_grad (component c of row i: k_handle w_i sum_a b_a p_{v_a, c} over the corners whose dof
 *     (v_a, c) is free), the "k_handle" key (-sum_i w_i sum_a b_a sum_{c free} p_{v_a, c} (p_i - t_i)_c), tsl_set_handle_frames, tsl_set_frame_poses,
 *     tsl_frame_wrench and tsl_frame_grad (the same six sums over these rows), tsl_energy, tsl_assemble, tsl_step, tsl_adjoint_step, both group steps. */
int tsl_set_handles_on_faces(tsl_ctx* ctx, const int32_t* faces_host, const double* bary_host, const double* weights_host, int32_t n);
int tsl_handle_points(tsl_ctx* ctx, const double* pos_dev, double* out_host);

/* Rigid frames for the handles (no reference counterpart): handle i may belong to frame f_i in [0, n_frame) with a local point r_i; f_i = -1 is a
 * free handle with a world target, as above.  Frame j has a pose (c_j, q_j), q = (s, x, y, z) in the convention of quat_to_rotmat
 * (engine/gripper_single.py), and the target of a framed handle is t_i = c_j + R(q_j) r_i.  Frames only rewrite rows of the target buffer: energy,
 * gradient, matrix, "k_handle", tsl_handle_force and tsl_handle_grad read the targets as before, and no frame kernel runs inside tsl_step,
 * tsl_energy, tsl_assemble or tsl_adjoint_step.  Conventions of tsl_set_handles: host pointers, the stream is synchronised, the lists are copied.
 *   tsl_set_handle_frames: frame_of_handle_host (n_handle), local_host (n_handle x 3; rows of free handles are not read), n_frame; n_frame = 0
 *     removes all frames and reads no list.  Fails, naming the offender, for a frame index outside [-1, n_frame), a non-finite local point of a
 *     framed handle, frames asked for while there are no handles.  Poses start at the identity at the origin, and the framed rows of the targets
 *     are written at once (t_i = r_i).  tsl_set_handles removes all frames: the handle list changed.
 *   tsl_set_frame_poses: pos_host (n_frame x 3), quat_host (n_frame x 4).  Every quaternion is normalised on the host; a zero or non-finite one
 *     (or a non-finite position) fails and names the frame.  Rewrites the rows of the targets that belong to framed handles; rows of free handles
 *     keep their value.  tsl_set_handle_targets on a context with frames uploads all rows and rewrites the framed ones again, so the targets do
 *     not depend on the order of the two calls.
 *   tsl_handle_targets: out_host (n_handle x 3) = the targets as they stand.
 *   tsl_frame_wrench: out_host (n_frame x 6) = (sum_i f_i, sum_i (t_i - c_j) x f_i) over the handles of frame j, f_i the row of tsl_handle_force:
 *     force and moment about c_j that the frame's handles apply to the cloth, = dE_h / d(c_j, theta_j).  Frozen dofs are NOT masked.
 *   tsl_frame_grad: the contribution of one reverse step to d(loss)/d(c_j) and d(loss)/d(theta_j), theta_j a world-frame rotation vector applied on
 *     the left (R <- exp([d theta]x) R): out_host (n_frame x 6) = (sum_i g_i, sum_i (R r_i) x g_i), g_i the row of tsl_handle_grad (k_handle w_i
 *     p_{v_i} on free dofs, 0 on frozen ones), sign of tsl_param_grad_keys; p_dev == NULL: the solution of the last tsl_adjoint_step.  Like
 *     tsl_handle_grad it belongs to the targets as last set: set the poses of step s before the reverse step s.
 *   Both read-outs: one workgroup per frame, a fixed order of additions (the same bits run to run); a frame without handles reads six zeros; with
 *     k_handle = 0 both read zeros and launch nothing; without frames both do nothing. */
int tsl_set_handle_frames(tsl_ctx* ctx, const int32_t* frame_of_handle_host, const double* local_host, int32_t n_frame);
int tsl_set_frame_poses(tsl_ctx* ctx, const double* pos_host, const double* quat_host);
int tsl_handle_targets(tsl_ctx* ctx, double* out_host);
int tsl_frame_wrench(tsl_ctx* ctx, const double* pos_dev, double* out_host);
int tsl_frame_grad(tsl_ctx* ctx, const double* p_dev, double* out_host);

/* Ties (no reference counterpart): tie i is a spring between vertex vertices[i] and the point with barycentric coordinates b_i on face faces[i] =
 * (t0, t1, t2) of the scene's global face table -- a seam between two cloths, a cloth sewn into a tube, a cloth on a point of a body's surface, a
 * tether.  r_i = x_v - sum_a b_a x_{t_a}, E_tie = 1/2 k_tie sum_i w_i |r_i|^2 with the scalar "k_tie" of tsl_set_param (0 by default; negative
 * fails).  In the order (t0, t1, t2, v) with c = (-b0, -b1, -b2, 1): gradient on corner a: k_tie w_i c_a r_i; block: k_tie w_i (c c^T) (x) I_3,
 * constant and positive semi-definite as it stands, so every spd mode and "spd_literal" add the same numbers.  b = (1, 0, 0) is a vertex-to-vertex
 * stitch.  A tie couples vertices that share no element: while ties exist and k_tie != 0 they are constraint slots behind the vertex-triangle and
 * edge-edge ones of the last detection (tsl_constraints_export, tsl_contact_blocks_export list them last; read with room for max_n_constraints + n
 * slots), at every step, with contacts on or off, and the plans of the factorisation hold their cliques.  The energy depends on the current
 * positions only: a reverse step carries nothing from a tie into the earlier steps.  Frozen dofs follow the mask rule.  With no ties or k_tie = 0
 * every launch is the one of a context that never had any.  No atomics, fixed orders of addition: the same bits run to run.
 *   tsl_set_ties: n ties (host pointers, copied; the stream is synchronised); weights_host == NULL: every weight is 1; n = 0 removes them.  Fails,
 *     naming the offender (tie, face, vertex), and leaves the previous list in place for a face outside [0, tot_NF), a vertex outside [0, tot_NV),
 *     a vertex that is a corner of its own face, a coordinate that is not finite or outside [0, 1], a triple that does not sum to 1 within 1e-9
 *     (coordinates are used as given), a negative or non-finite weight.  A member of a scene group cannot take a longer list than it had when the
 *     group was created: set the ties first.
 *   tsl_tie_count: n.  tsl_contact_counts keeps its two numbers.
 *   tsl_tie_force: out_host (n x 3) = -k_tie w_i r_i, the force tie i applies to its vertex at the state pos; frozen dofs are NOT masked.
 *   tsl_tie_residuals: out_host (n x 3) = r_i.
 *   tsl_tie_grad: out_host (n) = k_tie g_i, g_i = -sum_a sum_{c free} p_{a, c} c_a r_{i, c} at the tape state pos: the contribution of one reverse
 *     step to d(loss)/d(w_i), sign of tsl_param_grad_keys; p_dev == NULL: the solution of the last tsl_adjoint_step.  The "k_tie" key of
 *     tsl_param_grad_keys is sum_i w_i g_i. */
int tsl_set_ties(tsl_ctx* ctx, const int32_t* vertices_host, const int32_t* faces_host, const double* bary_host, const double* weights_host, int32_t n);
int tsl_tie_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_tie_force(tsl_ctx* ctx, const double* pos_dev, double* out_host);
int tsl_tie_residuals(tsl_ctx* ctx, const double* pos_dev, double* out_host);
int tsl_tie_grad(tsl_ctx* ctx, const double* pos_dev, const double* p_dev, double* out_host);

/* Half-space colliders (no reference counterpart: its tables are frozen bodies): up to TSL_MAX_COLLIDERS planes.  Collider j has a unit normal n_j,
 * fixed once the list is set, an offset o_j that may be set before every step -- the solid side is n_j . x < o_j --, and a friction coefficient
 * mu_j >= 0; the stiffness "k_collider" of tsl_set_param is shared (0 by default: off), the thickness of the shell is eps_contact, the friction
 * regularisation eps_v dt.  A per-vertex 8-bit mask says which colliders act on a vertex.  For vertex v and collider j, with x_prev the
 * start-of-step positions (the prev_pos argument of tsl_energy / tsl_assemble; x_{s-1} in a reverse step):
 *   d = n . x - o,  d0 = n . x_prev - o,  lam = mu k max(0, eps - d0),  u = T^T (x - x_prev),  r = |u|  (T from n as the contact pairs build theirs)
 *   E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r),  g = [d < eps] k (d - eps) n + lam f1(r) T u,
 *   H = [d < eps] k n n^T + lam T (f1 I + [r > 1e-9] (f2 / r) u u^T) T^T  on the vertex's own diagonal block,
 * positive semi-definite as it stands: every spd mode and "spd_literal" add the same numbers.  No constraint slot, no row list: the plans of the
 * factorisation and tsl_contact_counts do not depend on colliders.  A plane that moves along its own normal adds no slip.  Nothing is stored per
 * step; the normal term is evaluated at every evaluation.  Frozen dofs follow the mask rule.  One lane per vertex, no atomics: the same bits run
 * to run.  With no colliders or k_collider = 0 every launch is the one it was.
 *   tsl_set_colliders: normals_host (n x 3; normalised here), offsets_host (n), mu_host (n), vertex_mask_host (tot_NV bytes, bit j: collider j acts
 *     on the vertex; NULL: every collider on every vertex); host pointers, copied; the stream is synchronised; n = 0 removes the colliders.  Fails,
 *     naming the offender, and leaves the previous list in place for more than TSL_MAX_COLLIDERS colliders, a zero or non-finite normal, a
 *     non-finite offset, a negative or non-finite mu, a mask byte that names a collider at or above n.
 *   tsl_set_collider_offsets: offsets_host (n) for the next energy, assemble, step or adjoint step; set the offsets of step s before the reverse
 *     step s and before tsl_collider_grad.  A non-finite offset fails, naming the collider, and leaves the offsets in place.
 *   tsl_collider_count: n.
 *   tsl_collider_force: out_host (n x 3) = -sum_v g_v of collider j at the state (pos, prev_pos): the net force between plane j and the cloth, in the sign of
 *     tsl_handle_force (what the plane applies to the cloth: + m g along n under a resting cloth); frozen dofs are NOT masked; k_collider = 0: zeros.
 *   tsl_collider_grad: out_host (n x 2) at the tape state (pos = x_s, prev_pos = x_{s-1}), sign of tsl_handle_grad: column 0 the share of one
 *     reverse step in d(loss)/d(o_j at step s), -sum_v p_v . (-[d < eps] k n_j + [d0 < eps] mu_j k f1 T u); column 1 the share in d(loss)/d(mu_j),
 *     -sum_v p_v . (k max(0, eps - d0) f1 T u); free dofs only; p_dev == NULL: the solution of the last tsl_adjoint_step.  The reverse step itself
 *     adds H_f p_v + [d0 < eps] mu_j k (p_v . f1 T u) n_j (H_f the friction part of H) to the free dofs of the vertex's row of pos_grad[s-1]. */
#define TSL_MAX_COLLIDERS 8
int tsl_set_colliders(tsl_ctx* ctx, const double* normals_host, const double* offsets_host, const double* mu_host, int32_t n, const uint8_t* vertex_mask_host);
int tsl_set_collider_offsets(tsl_ctx* ctx, const double* offsets_host);
int tsl_collider_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_collider_force(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, double* out_host);
int tsl_collider_grad(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* p_dev, double* out_host);

/* Sphere colliders (no reference counterpart: its balls are meshed bodies): up to TSL_MAX_SPHERES solid balls with the cloth outside.  Sphere j has a
 * centre c_j that may be set before every step, a previous centre cp_j (where the ball was at the start of the step), a radius R_j > 0, fixed once
 * the list is set, and a friction coefficient mu_j >= 0; the stiffness "k_sphere" of tsl_set_param is shared (0 by default: off), the thickness of
 * the shell is eps_contact, the friction regularisation eh = eps_v dt.  A per-vertex 8-bit mask of its own says which spheres act on a vertex.  For
 * vertex v and sphere j, with x_prev the start-of-step positions (the prev_pos argument of tsl_energy / tsl_assemble; x_{s-1} in a reverse step):
 *   q  = x - c,       rho  = |q|,  n  = q / rho,   d  = rho - R
 *   q0 = x_prev - cp, rho0 = |q0|, n0 = q0 / rho0, d0 = rho0 - R
 *   lam = mu k max(0, eps - d0),  P0 = I - n0 n0^T,  D = (x - x_prev) - (c - cp),  w = P0 D,  r = |w|,  a = f1(r)
 *   E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r),  g = [d < eps] k (d - eps) n + lam a w,
 *   H = H_n + lam M on the vertex's own diagonal block,  H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T)),
 *   M = a P0 + [r > 1e-9] (f2 / r) w w^T.
 * The slip is relative to the ball: a ball that moves sideways drags the cloth, one that moves along n0 adds no slip.  The second part of H_n is
 * negative in the tangent plane: tsl_assemble with spd = 0 (the reverse step's operator) adds H_n exact, every other mode, with and without
 * "spd_literal", adds [d < eps] k n n^T (the eigen-clamp in closed form) and the same numbers; lam M is positive semi-definite as it stands.  No
 * constraint slot, no row list: the plans of the factorisation and tsl_contact_counts do not depend on spheres.  Nothing is stored per step.  A
 * pair with rho < 1e-12 contributes nothing, one with rho0 < 1e-12 has no friction.  Frozen dofs follow the mask rule.  One lane per vertex, no
 * atomics: the same bits run to run.  With no spheres or k_sphere = 0 every launch is the one it was.
 *   tsl_set_spheres: centres_host (n x 3), radii_host (n), mu_host (n), vertex_mask_host (tot_NV bytes, bit j: sphere j acts on the vertex; NULL:
 *     every sphere on every vertex); host pointers, copied; cp := c; the stream is synchronised; n = 0 removes the spheres.  Fails, naming the
 *     offender, and leaves the previous list in place for more than TSL_MAX_SPHERES spheres or n < 0, a non-finite centre, a radius that is not
 *     finite and positive, a negative or non-finite mu, a mask byte that names a sphere at or above n.
 *   tsl_set_sphere_centres: centres_host (n x 3) and prev_centres_host (n x 3; NULL: cp := c) for the next energy, assemble, step or adjoint step;
 *     set those of step s before the reverse step s and before tsl_sphere_grad.  A non-finite entry fails, naming the sphere, and leaves both in place.
 *   tsl_sphere_count: n.
 *   tsl_sphere_force: out_host (n x 3) = -sum_v g_v of sphere j at the state (pos, prev_pos): the net force the ball applies to the cloth, in the
 *     sign of tsl_collider_force; frozen dofs are NOT masked; k_sphere = 0: zeros.
 *   tsl_sphere_grad: out_host (n x 8) at the tape state (pos = x_s, prev_pos = x_{s-1}), sign of tsl_collider_grad, p the adjoint solution on its free
 *     dofs (p_dev == NULL: the solution of the last tsl_adjoint_step): the share of one reverse step in
 *       [0:3] d(loss)/d(c_j)  = -sum_v (dg/dc)^T p_v = sum_v (H_n + lam M) p_v  (H_n exact),
 *       [3:6] d(loss)/d(cp_j) = -sum_v (dg/dcp)^T p_v = -sum_v (lam M - L)^T p_v,
 *       [6]   d(loss)/d(mu_j) = -sum_v p_v . k max(0, eps - d0) a w,
 *       [7]   d(loss)/d(R_j)  = -sum_v p_v . (-[d < eps] k n + [d0 < eps] mu k a w),
 *     with L = dg/d(q0) at fixed D = -[d0 < eps] mu k (a w) n0^T + lam J_n P0 / rho0,  J_n = -B ((n0 . D) I + n0 D^T),  B = a I + [r > 1e-9] (f2 / r) w w^T.
 *     The reverse step itself adds -(dg/dx_prev)^T p_v = lam M p_v - L^T p_v to the free dofs of the vertex's row of pos_grad[s-1]. */
#define TSL_MAX_SPHERES 8
int tsl_set_spheres(tsl_ctx* ctx, const double* centres_host, const double* radii_host, const double* mu_host, int32_t n, const uint8_t* vertex_mask_host);
int tsl_set_sphere_centres(tsl_ctx* ctx, const double* centres_host, const double* prev_centres_host);
int tsl_sphere_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_sphere_force(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, double* out_host);
int tsl_sphere_grad(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* p_dev, double* out_host);

/* Capsule colliders (no reference counterpart: its rods are meshed bodies): up to TSL_MAX_CAPSULES solid rods with round ends and the cloth outside.
 * Capsule j has endpoints a_j, b_j that may be set before every step, previous endpoints ap_j, bp_j (where the rod was at the start of the step), a
 * radius R_j > 0, fixed once the list is set, and a friction coefficient mu_j >= 0; the stiffness "k_capsule" of tsl_set_param is shared (0 by
 * default: off), the thickness of the shell is eps_contact, the friction regularisation eh = eps_v dt.  A per-vertex 8-bit mask of its own says
 * which capsules act on a vertex.  The endpoints are independent: the rod may translate, rotate and change its length.  For vertex v and capsule
 * j, with x_prev the start-of-step positions (the prev_pos argument of tsl_energy / tsl_assemble; x_{s-1} in a reverse step):
 *   e  = b - a,    s  = (x - a) . e / (e . e),           t  = clamp(s, 0, 1),   in  = [0 < s < 1],   u  = e / |e|
 *   c  = a + t e,  q  = x - c,  rho = |q|,  n = q / rho,  d = rho - R
 *   e0 = bp - ap,  s0 = (x_prev - ap) . e0 / (e0 . e0),  t0 = clamp(s0, 0, 1),  in0 = [0 < s0 < 1],  u0 = e0 / |e0|
 *   c0 = ap + t0 e0,  q0 = x_prev - c0,  rho0, n0, d0 = rho0 - R
 *   lam = mu k max(0, eps - d0),  D = (x - x_prev) - ((1 - t0)(a - ap) + t0 (b - bp)),  P0 = I - n0 n0^T,  w = P0 D,  r = |w|,  a1 = f1(r)
 *   E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r),  g = [d < eps] k (d - eps) n + lam a1 w,
 *   H = H_n + lam M on the vertex's own diagonal block,  H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T - in u u^T)),
 *   M = a1 P0 + [r > 1e-9] (f2 / r) w w^T.
 * The slip is relative to the material point of the rod under the vertex at the start of the step: a rod that turns drags the cloth differently
 * along its length.  t0, n0 and lam are constants of the step.  tsl_assemble with spd = 0 (the reverse step's operator) adds H_n exact, every other
 * mode, with and without "spd_literal", adds [d < eps] k n n^T (the eigen-clamp in closed form: the eigenvectors are n, u and n x u); lam M is
 * positive semi-definite as it stands.  No constraint slot, no row list: the plans of the factorisation and tsl_contact_counts do not depend on
 * capsules.  Nothing is stored per step.  A pair with rho < 1e-12 contributes nothing, one with rho0 < 1e-12 has no friction.  Frozen dofs follow
 * the mask rule.  One lane per vertex, no atomics: the same bits run to run.  With no capsules or k_capsule = 0 every launch is the one it was.
 *   tsl_set_capsules: a_host, b_host (n x 3 each), radii_host (n), mu_host (n), vertex_mask_host (tot_NV bytes, bit j: capsule j acts on the vertex;
 *     NULL: every capsule on every vertex); host pointers, copied; ap := a, bp := b; the stream is synchronised; n = 0 removes the capsules.  Fails,
 *     naming the offender, and leaves the previous list in place for more than TSL_MAX_CAPSULES capsules or n < 0, a non-finite endpoint, a segment
 *     |b - a| shorter than 1e-9 m (a ball is what tsl_set_spheres is for), a radius that is not finite and positive, a negative or non-finite mu, a
 *     mask byte that names a capsule at or above n.
 *   tsl_set_capsule_ends: a_host, b_host and prev_a_host, prev_b_host (n x 3 each; both NULL: ap := a, bp := b; exactly one NULL fails) for the
 *     next energy, assemble, step or adjoint step; set those of step s before the reverse step s and before tsl_capsule_grad.  A non-finite entry
 *     or a segment or previous segment shorter than 1e-9 m fails, naming the capsule, and leaves all four in place.
 *   tsl_capsule_count: n.
 *   tsl_capsule_force: out_host (n x 6) at the state (pos, prev_pos): [0:3] -sum_v g_v of capsule j, the net force the rod applies to the cloth, in
 *     the sign of tsl_sphere_force; [3:6] -sum_v (x_v - m) x g_v with m = (a + b) / 2, its torque about the rod's midpoint in the same sign; frozen
 *     dofs are NOT masked; k_capsule = 0: zeros.
 *   tsl_capsule_grad: out_host (n x 14) at the tape state (pos = x_s, prev_pos = x_{s-1}), sign of tsl_sphere_grad, p the adjoint solution on its
 *     free dofs (p_dev == NULL: the solution of the last tsl_adjoint_step): the share of one reverse step in
 *       [0:3]  d(loss)/d(a_j)  = -sum_v (dg/da)^T p_v,    dg/da = -(1 - t) H_n + phi' tau n^T - (1 - t0) lam M   (H_n exact),
 *       [3:6]  d(loss)/d(b_j)  = -sum_v (dg/db)^T p_v,    dg/db = -t H_n - phi' tau n^T - t0 lam M,
 *       [6:9]  d(loss)/d(ap_j) = -sum_v (dg/dap)^T p_v,   [9:12] d(loss)/d(bp_j) = -sum_v (dg/dbp)^T p_v,
 *       [12]   d(loss)/d(mu_j) = -sum_v p_v . k max(0, eps - d0) a1 w,
 *       [13]   d(loss)/d(R_j)  = -sum_v p_v . (-[d < eps] k n + [d0 < eps] mu k a1 w),
 *     with phi' = [d < eps] k (d - eps), tau = in e / (e . e), tau0 = in0 e0 / (e0 . e0), Delta = (b - bp) - (a - ap), B = a1 I + [r > 1e-9] (f2 / r) w w^T,
 *     J_n = -B ((n0 . D) I + n0 D^T), G0 = I - n0 n0^T - in0 u0 u0^T and
 *       lagged(dd0, dn0, dt0, dD) = -[d0 < eps] mu k (a1 w) dd0^T + lam (M (dD - Delta dt0^T) + J_n dn0),
 *       dg/dx_prev = lagged(n0, G0 / rho0, tau0, -I),
 *       dg/dap = lagged(-(1 - t0) n0, -(1 - t0) G0 / rho0 + tau0 n0^T, in0 (-q0 - (1 - s0) e0) / (e0 . e0), (1 - t0) I),
 *       dg/dbp = lagged(-t0 n0, -t0 G0 / rho0 - tau0 n0^T, in0 (q0 - s0 e0) / (e0 . e0), t0 I).
 *     The reverse step itself adds -(dg/dx_prev)^T p_v to the free dofs of the vertex's row of pos_grad[s-1]. */
#define TSL_MAX_CAPSULES 8
int tsl_set_capsules(tsl_ctx* ctx, const double* a_host, const double* b_host, const double* radii_host, const double* mu_host, int32_t n, const uint8_t* vertex_mask_host);
int tsl_set_capsule_ends(tsl_ctx* ctx, const double* a_host, const double* b_host, const double* prev_a_host, const double* prev_b_host);
int tsl_capsule_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_capsule_force(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, double* out_host);
int tsl_capsule_grad(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* p_dev, double* out_host);

/* Rounded-box colliders (no reference counterpart: its table tops are meshed bodies): up to TSL_MAX_BOXES solid boxes with rounded edges and corners
 * and the cloth outside -- a table top whose edge the cloth hangs over, a shelf, a step, a gripper jaw, a plate that tilts.  Box j has a centre c_j
 * and an orientation that may be set before every step, a previous pose (where the box was at the start of the step), half extents h_j >= 0 of the
 * core box and a rounding radius r_j > 0 (the solid is the core box grown by r_j; no sharp box), both fixed once the list is set, and a friction
 * coefficient mu_j >= 0; the stiffness "k_box" of tsl_set_param is shared (0 by default: off), the thickness of the shell is eps_contact, the
 * friction regularisation eh = eps_v dt.  A per-vertex 8-bit mask of its own says which boxes act on a vertex.  Poses are a centre and a quaternion
 * (s, x, y, z), normalised by the library and turned into R (columns u_i: the box axes in the world) once on the host.  For vertex v and box j,
 * with x_prev the start-of-step positions (the prev_pos argument of tsl_energy / tsl_assemble; x_{s-1} in a reverse step):
 *   y  = R^T (x - c),        b  = clamp(y, -h, h),    free_i  = [-h_i < y_i < h_i]   (an axis with h_i = 0 is never free)
 *   q  = R (y - b),  rho = |q|,  n = q / rho,  d = rho - r
 *   y0 = R0^T (x_prev - cp), b0 = clamp(y0, -h, h),   free0_i = [-h_i < y0_i < h_i]
 *   q0 = R0 (y0 - b0), rho0, n0, d0 = rho0 - r
 *   lam = mu k max(0, eps - d0),  dc = (c + R b0) - (cp + R0 b0),  D = (x - x_prev) - dc,  P0 = I - n0 n0^T,  w = P0 D,  r_w = |w|,  a1 = f1(r_w)
 *   E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r_w),  g = [d < eps] k (d - eps) n + lam a1 w,
 *   H = H_n + lam M on the vertex's own diagonal block,  H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T - sum_i free_i u_i u_i^T)),
 *   M = a1 P0 + [r_w > 1e-9] (f2 / r_w) w w^T.
 * The slip is relative to the material point of the box under the vertex at the start of the step: a plate that tilts drags the cloth with it.
 * b0, n0 and lam are constants of the step.  The curvature term vanishes on a face, is the rod's on an edge and the ball's at a corner: half
 * extents (L/2, 0, 0) give the capsule of length L, (0, 0, 0) the sphere.  tsl_assemble with spd = 0 (the reverse step's operator) adds H_n exact,
 * every other mode, with and without "spd_literal", adds [d < eps] k n n^T (the eigen-clamp in closed form); lam M is positive semi-definite as it
 * stands.  No constraint slot, no row list: the plans of the factorisation and tsl_contact_counts do not depend on boxes.  Nothing is stored per
 * step.  A pair with rho < 1e-12 (a vertex inside the core box, deeper than r) contributes nothing, one with rho0 < 1e-12 has no friction: the
 * limit of the model.  Frozen dofs follow the mask rule.  One lane per vertex, no atomics: the same bits run to run.  With no boxes or k_box = 0
 * every launch is the one it was.
 *   tsl_set_boxes: centres_host (n x 3), quats_host (n x 4), half_extents_host (n x 3), radii_host (n), mu_host (n), vertex_mask_host (tot_NV bytes,
 *     bit j: box j acts on the vertex; NULL: every box on every vertex); host pointers, copied; the previous poses := the poses; the stream is
 *     synchronised; n = 0 removes the boxes.  Fails, naming the offender, and leaves the previous list in place for more than TSL_MAX_BOXES boxes or
 *     n < 0, a non-finite centre, a zero or non-finite quaternion, a negative or non-finite half extent, a radius that is not finite and positive,
 *     a negative or non-finite mu, a mask byte that names a box at or above n.
 *   tsl_set_box_poses: centres_host, quats_host and prev_centres_host, prev_quats_host (both NULL: the previous poses := the poses; exactly one
 *     NULL fails) for the next energy, assemble, step or adjoint step; set those of step s before the reverse step s and before tsl_box_grad.  A
 *     non-finite centre or a zero or non-finite quaternion fails, naming the box, and leaves all four in place.
 *   tsl_box_count: n.
 *   tsl_box_force: out_host (n x 6) at the state (pos, prev_pos): [0:3] -sum_v g_v of box j, the net force the box applies to the cloth, in the
 *     sign of tsl_sphere_force; [3:6] -sum_v (x_v - c) x g_v, its torque about the box's centre in the same sign; frozen dofs are NOT masked;
 *     k_box = 0: zeros.
 *   tsl_box_grad: out_host (n x 14) at the tape state (pos = x_s, prev_pos = x_{s-1}), sign of tsl_sphere_grad, p the adjoint solution on its
 *     free dofs (p_dev == NULL: the solution of the last tsl_adjoint_step): the share of one reverse step in
 *       [0:3]  d(loss)/d(c_j)       = sum_v H_n p_v + lam M p_v   (H_n exact),
 *       [3:6]  d(loss)/d(theta_j)   = sum_v (x - c) x (H_n p_v) + p_v x g_n + (R b0) x (lam M p_v),   g_n = [d < eps] k (d - eps) n,
 *       [6:9]  d(loss)/d(cp_j)      = -sum_v X,
 *       [9:12] d(loss)/d(theta_p_j) = sum_v -(x_prev - cp) x X - lam n0 x z + lam q0 x (M p_v),
 *       [12]   d(loss)/d(mu_j)      = -sum_v p_v . k max(0, eps - d0) a1 w,
 *       [13]   d(loss)/d(r_j)       = -sum_v p_v . (-[d < eps] k n + [d0 < eps] mu k a1 w),
 *     with theta, theta_p world-frame rotation vectors applied on the left (R <- exp([theta]x) R, as tsl_frame_grad), B = a1 I + [r_w > 1e-9]
 *     (f2 / r_w) w w^T, z = -((n0 . D) B p_v + D (n0 . B p_v)), G0 = P0 - sum_i free0_i u0_i u0_i^T, Delta = sum_i free0_i (u_i - u0_i) u0_i^T and
 *       X = lam (M p_v - G0 z / rho0) + [d0 < eps] mu k n0 (a1 w . p_v) + lam Delta^T M p_v = -(dg/dx_prev)^T p_v,
 *     which the reverse step itself adds to the free dofs of the vertex's row of pos_grad[s-1].  There is no gradient for the half extents. */
#define TSL_MAX_BOXES 8
int tsl_set_boxes(tsl_ctx* ctx, const double* centres_host, const double* quats_host, const double* half_extents_host, const double* radii_host, const double* mu_host, int32_t n,
                  const uint8_t* vertex_mask_host);
int tsl_set_box_poses(tsl_ctx* ctx, const double* centres_host, const double* quats_host, const double* prev_centres_host, const double* prev_quats_host);
int tsl_box_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_box_force(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, double* out_host);
int tsl_box_grad(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* p_dev, double* out_host);

/* Wind (no reference counterpart, which has no load from the medium): lagged linear aerodynamic drag on a list of cloth faces.  Wind face f of the
 * list has the corners (v_0, v_1, v_2) of its face in the scene's face table (faces_host of tsl_scene_desc; the cloths' faces are its first
 * sum NF faces) and a weight w_f >= 0; the coefficients "wind_cn" (normal) and "wind_ct" (tangential) of tsl_set_param, both in N s / m^3 and 0 by
 * default, are shared, and there is one wind velocity W per step and scene.  With x_prev the start-of-step positions (the prev_pos argument of
 * tsl_energy / tsl_assemble; x_{s-1} in a reverse step):
 *   a   = 1/2 (xp_1 - xp_0) x (xp_2 - xp_0),  A0 = |a|,  n0 = a / A0          the lagged area vector
 *   M   = w_f [ c_t A0 I + (c_n - c_t) a a^T / A0 ] = w_f A0 (c_n n0 n0^T + c_t (I - n0 n0^T))
 *   r   = (xbar - xpbar) / dt - W,  xbar = (x_0 + x_1 + x_2) / 3
 *   E_w = dt / 2 sum_f r^T M r,  gradient row of each corner: M r / 3,  block of each of the nine corner pairs: M / (9 dt).
 * The force on the sheet is M (W - u) with u the centroid's velocity over the step.  M depends on x_prev only: the blocks are constant over the
 * Newton iterations of a step and positive semi-definite as they stand, so every spd mode, with and without "spd_literal", adds the same numbers.
 * The three pair blocks of a cloth face are in the matrix pattern already: no constraint slot, no row list, and the plans of the factorisation and
 * tsl_contact_counts do not depend on the wind.  A face with A0 < 1e-12 m^2 at the start of the step contributes nothing.  Frozen dofs follow the
 * mask rule.  One record per face, then one lane per touched vertex and per touched block over gather lists, no atomics: the same bits run to run.
 * With no list, or wind_cn = wind_ct = 0, every launch is the one it was.  Not modelled: drag quadratic in speed; a wind that varies in space (the
 * weights are the only spatial handle); faces of FEM bodies (refused); gradients for the weights; keys of tsl_param_grad_keys (the coefficient
 * columns of tsl_wind_grad carry those gradients).
 *   tsl_set_wind: faces_host (n global face ids), weights_host (n; NULL: 1 each); host pointers, copied; the stream is synchronised; n = 0 removes
 *     the list; faces_host == NULL with n = -1: every cloth face in ascending order (weights_host then has one entry per cloth face).  Fails, naming
 *     the offender, and leaves the previous list in place for n < 0, a face out of range, a surface face of a body, a face listed twice, a
 *     negative or non-finite weight.
 *   tsl_set_wind_velocity: W_host (3) for the next energy, assemble, step or adjoint step; set that of step s before the reverse step s and before
 *     tsl_wind_grad.  A non-finite component fails, naming it, and leaves the velocity in place.
 *   tsl_wind_count: n.
 *   tsl_wind_force: out_host (3) = -sum_f M_f r_f at the state (pos, prev_pos): the net force the wind applies to the cloth; frozen dofs are NOT
 *     masked; wind off: zeros.
 *   tsl_wind_grad: out_host (5) at the tape state (pos = x_s, prev_pos = x_{s-1}), sign of tsl_sphere_grad, p the adjoint solution on its free
 *     dofs (p_dev == NULL: the solution of the last tsl_adjoint_step), P_f its sum over the corners of face f: the share of one reverse step in
 *       [0:3] d(loss)/d(W)   = +1/3 sum_f M_f P_f,
 *       [3]   d(loss)/d(c_n) = -1/3 sum_f w_f A0 (n0.r)(n0.P_f),
 *       [4]   d(loss)/d(c_t) = -1/3 sum_f w_f A0 (r.P_f - (n0.r)(n0.P_f)).
 *     The reverse step itself adds -(dg/dx_prev)^T p to the free dofs of the corners' rows of pos_grad[s-1]: M P_f / (9 dt) to each corner (through r)
 *     and, through a, with q = 1/3 w_f [ c_t (P.r) a / A0 + (c_n - c_t) (((a.r) P + (a.P) r) / A0 - (a.P)(a.r) a / A0^3) ], e1 = xp_1 - xp_0 and
 *     e2 = xp_2 - xp_0:  -1/2 (e2 x q) to corner 1, -1/2 (q x e1) to corner 2, minus their sum to corner 0. */
int tsl_set_wind(tsl_ctx* ctx, const int32_t* faces_host, const double* weights_host, int32_t n);
int tsl_set_wind_velocity(tsl_ctx* ctx, const double* W_host);
int tsl_wind_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_wind_force(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, double* out_host);
int tsl_wind_grad(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* p_dev, double* out_host);

/* Sampled distance-field colliders (no reference counterpart: its moulds are meshed bodies with every vertex frozen): up to TSL_MAX_SDFS solids
 * {phi < r} with the cloth outside, phi sampled on a grid -- a mould a sheet is formed into, a bowl, a ring, a shoulder, a jaw with a groove: any
 * solid, concave ones included.  Field j has dimensions (n0, n1, n2), each in [4, 512], one isotropic spacing h > 0, an origin o (the local position
 * of sample (0, 0, 0)) and n0 n1 n2 doubles in C order, at most 2^26 over the list, all fixed once the list is set; an offset r (any finite value),
 * a friction coefficient mu >= 0, and a pose (centre c, quaternion (s, x, y, z), normalised by the library) that may be set before every step, with
 * the previous pose cp, R0.  The stiffness "k_sdf" of tsl_set_param is shared (0 by default: off), the thickness of the shell is eps_contact, the
 * friction regularisation eh = eps_v dt.  A per-vertex 8-bit mask of its own says which fields act on a vertex.  phi is the tensor-product uniform
 * cubic B-spline over the samples (C2; its gradient is C1 everywhere, so the reverse step's operator is the exact second derivative of the energy):
 *   t = (y - o) / h,  i_a = floor(t_a),  f_a = t_a - i_a,   valid  <=>  1 <= t_a < n_a - 2 for a = 0, 1, 2   (in double; NaN is not valid)
 *   phi(y) = sum_{a,b,c in 0..3} B_a(f_0) B_b(f_1) B_c(f_2) s[i_0-1+a, i_1-1+b, i_2-1+c]
 *   B_0 = (1-f)^3/6,  B_1 = (3f^3 - 6f^2 + 4)/6,  B_2 = (-3f^3 + 3f^2 + 3f + 1)/6,  B_3 = f^3/6;  grad phi: one factor B' and 1/h;  Hess phi: B'' or
 *   B'B' and 1/h^2.
 * The samples are the control values: a sampled linear field is reproduced exactly, a constant added to the samples is added to phi, a curved field
 * is smoothed by about h^2/6 times its Laplacian.  For vertex v and field j, with x_prev the start-of-step positions:
 *   y  = R^T (x - c),        d  = phi(y) - r,    m  = R grad phi(y)   (not normalised: the energy is a function of phi itself)
 *   y0 = R0^T (x_prev - cp), d0 = phi(y0) - r,   s0 = |grad phi(y0)|,  n0 = R0 grad phi(y0) / s0
 *   lam = [y0 valid][s0 >= 1e-12] mu k max(0, eps - d0),  D = (x - c) - R y0 = (x - x_prev) - dc,  dc = (c - cp) + (R - R0) y0,
 *   P0 = I - n0 n0^T,  w = P0 D,  r_w = |w|,  a1 = f1(r_w),  M = a1 P0 + [r_w > 1e-9] (f2 / r_w) w w^T
 *   E = [y valid][d < eps] 1/2 k (d - eps)^2 + lam f0(r_w),  g = [y valid][d < eps] k (d - eps) m + lam a1 w,
 *   H = H_n + lam M on the vertex's own diagonal block,  H_n = [y valid][d < eps] k (m m^T + (d - eps) R Hess phi(y) R^T).
 * tsl_assemble with spd = 0 (the reverse step's operator) adds H_n exact; every other mode, with and without "spd_literal", adds
 * [y valid][d < eps] k m m^T, the Gauss-Newton part: positive semi-definite, but not the eigen-clamp of H_n (a general field has no closed-form clamp
 * worth its cost in a 3 x 3 block).  Outside the valid region a pair contributes nothing -- at x no normal term, at x_prev no friction --: a solid
 * that reaches the border of its grid ends there, and keeping it inside is the caller's business.  No constraint slot, no row list: the plans of
 * the factorisation and tsl_contact_counts do not depend on fields.  Nothing is stored per step.  Frozen dofs follow the mask rule.  One lane per
 * vertex, no atomics: the same bits run to run.  With no fields or k_sdf = 0 every launch is the one it was.  Not modelled: gradients for the
 * samples, a prefilter that makes the spline interpolate, anisotropic spacing, more than TSL_MAX_SDFS fields, any check that a solid stays inside its
 * grid.
 *   tsl_set_sdfs: samples_host (the fields' samples one after the other), dims_host (n x 3 int32), origins_host (n x 3), spacings_host (n),
 *     centres_host (n x 3), quats_host (n x 4), offsets_host (n), mu_host (n), vertex_mask_host (tot_NV bytes, bit j: field j acts on the vertex; NULL:
 *     every field on every vertex); host pointers, copied; the previous poses := the poses; the stream is synchronised; n = 0 removes the fields and
 *     frees the samples.  Fails, naming the offender, and leaves the previous list AND the previous samples in place for n < 0 or more than
 *     TSL_MAX_SDFS fields, a null array, a dimension below 4 or above 512, more than 2^26 samples in total, a spacing that is not finite and
 *     positive, a non-finite origin, offset, centre or sample (named by the field and its three indices), a zero or non-finite quaternion, a negative
 *     or non-finite mu, a mask byte that names a field at or above n.
 *   tsl_set_sdf_poses: centres_host, quats_host and prev_centres_host, prev_quats_host (both NULL: the previous poses := the poses; exactly one NULL
 *     fails) for the next energy, assemble, step or adjoint step; set those of step s before the reverse step s and before tsl_sdf_grad.  A
 *     non-finite centre or a zero or non-finite quaternion fails, naming the field, and leaves all four in place.
 *   tsl_sdf_count: n.
 *   tsl_sdf_force: out_host (n x 6) at the state (pos, prev_pos): [0:3] -sum_v g_v of field j, the net force the solid applies to the cloth;
 *     [3:6] -sum_v (x_v - c) x g_v, its torque about the field's centre in the same sign; frozen dofs are NOT masked; k_sdf = 0: zeros.
 *   tsl_sdf_grad: out_host (n x 14) at the tape state (pos = x_s, prev_pos = x_{s-1}), sign of tsl_box_grad, p the adjoint solution on its free
 *     dofs (p_dev == NULL: the solution of the last tsl_adjoint_step): the share of one reverse step in
 *       [0:3]  d(loss)/d(c_j)       = sum_v H_n p_v + lam M p_v   (H_n exact),
 *       [3:6]  d(loss)/d(theta_j)   = sum_v (x - c) x (H_n p_v) + p_v x g_n + (R y0) x (lam M p_v),   g_n = [y valid][d < eps] k (d - eps) m,
 *       [6:9]  d(loss)/d(cp_j)      = -sum_v X,
 *       [9:12] d(loss)/d(theta_p_j) = sum_v -(x_prev - cp) x X - lam n0 x z,
 *       [12]   d(loss)/d(mu_j)      = -sum_v p_v . k max(0, eps - d0) a1 w,
 *       [13]   d(loss)/d(r_j)       = -sum_v p_v . (-[d < eps] k m + [d0 < eps] mu k a1 w),
 *     with theta, theta_p world-frame rotation vectors applied on the left (R <- exp([theta]x) R, as tsl_box_grad), B = a1 I + [r_w > 1e-9]
 *     (f2 / r_w) w w^T, z = -((n0 . D) B p_v + D (n0 . B p_v)) and
 *       X = lam (R0 R^T M p_v - R0 Hess phi(y0) R0^T P0 z / s0) + [d0 < eps] mu k s0 n0 (a1 w . p_v) = -(dg/dx_prev)^T p_v,
 *     which the reverse step itself adds to the free dofs of the vertex's row of pos_grad[s-1].  There is no gradient for the samples. */
#define TSL_MAX_SDFS 8
int tsl_set_sdfs(tsl_ctx* ctx, const double* samples_host, const int32_t* dims_host, const double* origins_host, const double* spacings_host, const double* centres_host,
                 const double* quats_host, const double* offsets_host, const double* mu_host, int32_t n, const uint8_t* vertex_mask_host);
int tsl_set_sdf_poses(tsl_ctx* ctx, const double* centres_host, const double* quats_host, const double* prev_centres_host, const double* prev_quats_host);
int tsl_sdf_count(tsl_ctx* ctx, int32_t* out_host);
int tsl_sdf_force(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, double* out_host);
int tsl_sdf_grad(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* p_dev, double* out_host);

/* BaseScene.compute_energy (BaseScene.py:427-451) at the given state, constraints as last detected. */
int tsl_energy(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* vel_dev,
               const double* ref_angle_dev, double* energy_host);

/* newton_step_init + compute_residual_and_Hessian(spd) (BaseScene.py:976-1040) or, with grad_dev == NULL,
 * compute_Hessian(spd) (BaseScene.py:1042-1052).  grad_dev (3*tot_NV) receives BaseScene.F. */
int tsl_assemble(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, const double* vel_dev,
                 const double* ref_angle_dev, int spd, double* grad_dev);

/* SparseMatrix.solve (sparse_solver.py:85-105): x = H^-1 rhs for the matrix of the last tsl_assemble. */
int tsl_solve(tsl_ctx* ctx, const double* rhs_dev, double* x_dev, tsl_solve_stats* stats_host);

/* BaseScene.time_step (BaseScene.py:1327-1370; Scene_folding.py:279-322): contact detection, Newton loop with
 * halving line search, velocity update, optional plastic ref-angle update.  State arrays are updated in place. */
int tsl_step(tsl_ctx* ctx, double* pos_dev, double* prev_pos_dev, double* vel_dev, double* ref_angle_dev,
             tsl_step_stats* stats_host);

/* calc_vn + projection_query + contact_analysis (BaseScene.py:837-850, geometry.py:223-229, BaseScene.py:818-835).
 * proj_flag / proj_dir persist inside the context between calls (geometry.py:210-219). */
int tsl_contact_detect(tsl_ctx* ctx, const double* pos_dev, const double* prev_pos_dev, int32_t* nc_host);
int tsl_contact_reset(tsl_ctx* ctx); /* BaseScene.reset: proj_flag.fill(0) (BaseScene.py:268) */
/* {vertex-triangle, edge-edge} constraints of the last detection (their sum is tsl_step_stats.nc); the edge-edge ones ("contact_ee" = 1) are the
 * slots [out2[0], out2[0] + out2[1]) of the list.  Such a slot has idx = (b0, b1, a0, a1): target edge (b0, b1), query edge (a0, a1) in the order that
 * makes the signed line distance positive on the side the query edge was on at detection; w = (s, t, 0) with a(s) = (1 - s) x_a0 + s x_a1 and
 * b(t) = (1 - t) x_b0 + t x_b1 the closest points at detection; friction acts on a(s) - b(t) - dx0. */
int tsl_contact_counts(tsl_ctx* ctx, int32_t* out2_host);

/* Cloth.update_ref_angle (model_fold_offset.py:176-185) for every cloth. */
int tsl_update_ref_angle(tsl_ctx* ctx, const double* pos_dev, double* ref_angle_dev);

/* Grad.transfer_grad (analytic_grad_single.py:217-257) for one step s.  Buffers are the Grad fields:
 * pos_buffer/pos_grad (T x tot_NV x 3), ref_angle_buffer/angleref_grad (T x cloth_faces x 3).
 * On return tmp_z_frozen_dev (3*tot_NV) holds BaseScene.tmp_z_frozen for gripper.gather_grad. */
int tsl_adjoint_step(tsl_ctx* ctx, int step, int tot_timestep, const double* pos_buffer_dev, double* pos_grad_dev,
                     const double* ref_angle_buffer_dev, double* angleref_grad_dev, double* tmp_z_frozen_dev,
                     double adjoint_damping, tsl_solve_stats* stats_host);

/* Elastic.get_force of every FEM body (model_elastic_tactile.py:144-164, model_elastic_offset.py:188-208): internal force +
 * gravity + external force per vertex; consumed by BaseScene.check_early_stop / gather_force (BaseScene.py:1541-1584).
 * force_dev: tot_NV x 3, rows of the cloths are zero. */
int tsl_elastic_force(tsl_ctx* ctx, const double* pos_dev, double* force_dev);

/* System identification (engine/analytic_grad_system.py:112-160): the reverse step is tsl_adjoint_step with
 * tsl_set_param "adj_clamp" = 1 and "adj_clamp_angleref" = 0 (that class clamps pos_grad to +-1 and nothing else, :104-109);
 * this call then returns the sums over the free dofs of p . d(force)/d(parameter) with p the solution of that step
 * (get_parameters_grad :69-80 with BaseScene.get_paramters_grad BaseScene.py:1513-1525, Cloth.compute_deri
 * model_fold_offset.py:1082-1127, Elastic.compute_deri model_elastic_tactile.py:329-347 / model_elastic_offset.py:415-431).
 * pos = tape state x_s, ref_angle = tape rest angles of step s-1 (copy_pos_and_refangle, BaseScene.py:284-292).
 * out_host = {grad_kb, grad_mu, grad_lam} contributions of this step (grad_lam is 0: the reference never pushes d_lam up). */
int tsl_param_grad(tsl_ctx* ctx, const double* pos_dev, const double* ref_angle_dev, double* out_host);

/* Scene_sliding.contact_energy_backprop_friction (Scene_sliding.py:139-176): contribution of the last tsl_adjoint_step to
 * d(loss)/d(mu_cloth_cloth), summed over the constraints of the pairs that use that parameter. pos = tape state x_s.
 * Fails (< 0) while edge-edge constraints ("contact_ee" = 1) of such pairs are present: their term is not implemented. */
int tsl_friction_grad(tsl_ctx* ctx, const double* pos_dev, double* out_host);

/* d(loss)/d(theta) contributions of one reverse step for any of the material and contact scalars: out_host[j] = sum over the free dofs of
 * p . d(force)/d(theta_j) (force = -F, F the gradient tsl_assemble forms: the sign of tsl_param_grad, whose kb is the sum of the "cloth<i>.Kb"
 * values), theta_j = the value tsl_set_param(keys[j]) sets, every other key held fixed.
 * Keys: "cloth<i>.Kl", "cloth<i>.Ka", "cloth<i>.Kb", "cloth<i>.stvk_mu", "cloth<i>.stvk_lam" (StVK membrane, "cloth<i>.membrane" = 1), "elastic<i>.mu",
 * "elastic<i>.lam" (both material models, alpha fixed), "k_contact" (normal
 * term of every vertex-triangle slot and the friction weights c_k = -mu k_contact (gap - eps) of the detection), "mu_cloth_elastic",
 * "mu_cloth_cloth" (friction of the slots whose pair uses that live parameter, the pair's factor kept: d c_k = c_k / mu_live),
 * "k_handle" (soft handles: -sum_i w_i p_{v_i} . (x_{v_i} - t_i) over free dofs with the targets as last set; exactly 0 with no handles),
 * "k_tie" (ties: sum_i w_i g_i of tsl_tie_grad; exactly 0 with no ties; resolved ahead of the key table, its partial sums lie behind the table's) -- twelve key forms.
 * p_dev == NULL: the solution of the last tsl_adjoint_step (as tsl_param_grad uses it); otherwise any 3*tot_NV vector (original vertex order).
 * pos = tape state x_s, ref_angle = tape rest angles of step s-1 (needed by the Kb keys only); contact constraints as last detected / as the
 * last adjoint step left them -- c_k and dx0 are records of the detection, the derivative does not differentiate detection.
 * Fails (< 0, the key named in tsl_last_error) for an unknown or non-differentiated key (eps_contact, damping, k_angle, alpha, solver keys, ...),
 * a body index out of range, "k_contact" while edge-edge constraints ("contact_ee" = 1) are present, "mu_cloth_*" while an edge-edge
 * constraint of that parameter is present (their friction derivative is not implemented), and a contact key whose live value is 0 (the
 * derivative exists there, but the detection records c_k vanish with the value and cannot carry it: start a fit from a small nonzero value).
 * A key that does not enter F is exactly 0: "stvk_*" of a cloth with membrane = 0, "Kl" / "Ka" of a cloth with membrane = 1.
 * Deterministic: per-workgroup partials per key joined in a fixed order, a key's value is the same bits whichever other keys are asked for.
 * One device-to-host copy and one stream synchronisation per call. */
int tsl_param_grad_keys(tsl_ctx* ctx, const double* pos_dev, const double* ref_angle_dev, const double* p_dev, const char* const* keys,
                        int32_t n_keys, double* out_host);

/* Introspection used by the parity tests (tests/ only): assembled matrix as BSR on the host. */
int tsl_matrix_nnzb(tsl_ctx* ctx, int32_t* nb_host, int32_t* nnzb_host);
int tsl_matrix_export(tsl_ctx* ctx, int32_t* row_ptr_host, int32_t* col_host, double* vals_host);
/* The inverse of tsl_matrix_export (tests/ only): vals_host [nnzb][3][3] in exactly the pattern and order tsl_matrix_export returns
 * replaces the static part of the operator; the contact blocks of the last detection are kept.  The factors, |H|_inf, the multigrid
 * operators and a separate preconditioner matrix are marked stale, as tsl_assemble does; the values hold until the next assemble or step. */
int tsl_matrix_import(tsl_ctx* ctx, const double* vals_host);
int tsl_constraints_export(tsl_ctx* ctx, int32_t* idx_host, double* w_host, double* k_host, double* dx0_host,
                           double* T_host, double* n_host, double* mu_host, int32_t max_n);
/* per-constraint dense 12x12 blocks (vertex order idx0..idx3) of the last assemble; masked = frozen rule applied */
int tsl_contact_blocks_export(tsl_ctx* ctx, double* blocks_host, int32_t max_n, int32_t masked);
int tsl_proj_export(tsl_ctx* ctx, int32_t* proj_flag_host, int32_t* proj_dir_host, int32_t* proj_idx_host, double* proj_w_host);
int tsl_proj_import(tsl_ctx* ctx, const int32_t* proj_flag_host, const int32_t* proj_dir_host);
/* BaseScene.border_flag (tot_NV; BaseScene.py:104, restored by Scene_balancing.load_all :213-222, read by project_pair geometry.py:194-201) */
int tsl_set_border(tsl_ctx* ctx, const int32_t* border_flag_host);

/* Batched SPD projections (linalg.py:5-12 and :15-148) on device arrays of D x D blocks, D in {2,3,9}; D = 3 and 9 follow "spd_literal"
 * (the device functions of the assembly, K = 10 / 20). */
int tsl_spd_project(tsl_ctx* ctx, double* blocks_dev, int32_t n_blocks, int32_t D);

/* Timing of the dominant kernel for bench.py's roofline object: HIP-event time (ms) accumulated over the
 * PCG iteration kernels since the last reset, launch count and the bytes one iteration moves algorithmically.
 * Sampled launches (1 in 16) are timed twice: by the device wall clock inside the kernel (min start / max end over waves =
 * the duration a kernel trace reports) and by a hipEvent pair around the launch on the engine stream. */
int tsl_profile_reset(tsl_ctx* ctx, int enable);
int tsl_profile_read(tsl_ctx* ctx, double* spmv_ms_host, int64_t* spmv_launches_host, int64_t* spmv_bytes_per_launch_host);
int tsl_profile_read_events(tsl_ctx* ctx, double* spmv_ms_hip_events_host); /* same launches bracketed by hipEvents (includes launch gaps) */
/* `reps` back-to-back launches of one operator kernel on the currently assembled matrix (and the current step's contact rows),
 * bracketed by ONE hipEvent pair on the engine stream: average microseconds per launch.  variant 20 = k_pcg_spmv exactly as a
 * PCG iteration launches it (what bench.py's roofline object is priced on), 2 = the plain SELL-64 product k_spmv_mw,
 * 30 = k_stream_read over the matrix values only (streaming-read yardstick for the same bytes). */
int tsl_bench_spmv(tsl_ctx* ctx, int variant, int reps, double* us_per_launch_host);

/* Sparse direct path (multifrontal LU of the operator, the counterpart of the reference's spsolve, sparse_solver.py:85-105).
 * tsl_bench_direct: the launches of one kernel class of ONE factorisation (cls 0 the Gauss-Jordan inversions W = F11^-1 on the block-step
 * path: k_ds_pivot0 + k_ds_gj_step + k_ds_gj_finish; 1 k_ds_gemm in Schur mode: product, gather of the children's Schur complements,
 * store; 2 k_ds_gemm in G = W F12 mode; 3 the inversions in the LDS kernel k_ds_inv_small; 5 the inversions in the persistent dataflow
 * kernel k_ds_gj_flow; 6 k_ds_extend_panels, the panels' share of the extend-add) or of one application (4 k_ds_gemv) on the current
 * plan, replayed `reps` times between one hipEvent pair;
 * out4 = {us per launch, algorithmic flops per launch, algorithmic bytes per launch, launches per factorisation}.  The factors are
 * invalid afterwards.  tsl_direct_info: {plans, factorisations, applications, perturbed pivots of the last factorisation, host
 * seconds in plan builds, supernodes, levels, batches, flops per factorisation, bytes of fronts (panels + Schur complements)}.
 * tsl_direct_counters: the first n of {dataflow launches, dataflow launches that lost a flag (redone on the block-step path), plan-cache
 * hits, bytes of the panel arena (cleared per factorisation), of the Schur arena, of the G arena, Schur-complement entries stored per
 * factorisation, plans parked in the cache, first passes of refined solves whose normwise backward error |b - Hx| / (|H|_inf |x| + |b|)
 * was evaluated, first passes accepted on it ("direct_berr", default 1e-12), largest backward error / forward residual so accepted}. */
int tsl_bench_direct(tsl_ctx* ctx, int cls, int reps, double* out4_host);
int tsl_direct_info(tsl_ctx* ctx, double* out10_host);
int tsl_direct_counters(tsl_ctx* ctx, double* out_host, int32_t n);

/* ---- the iterative hierarchy taken apart (tests/ only): read-only views of the last preconditioner set-up, and entry points that run one
 * part of the hierarchy alone.  All four run the set-up a solve would run first if it is stale (block-Jacobi inverse, dense body inverses,
 * mg_setup_operators), launch no kernel a solve does not launch, and alter no state a solve does not alter.
 *   tsl_mg_info:   out = {cloth hierarchies H (0 with the multigrid off), dense bodies B (0 while they are not in use);
 *                  per hierarchy: v_offset, N0, M0, levels L the cycle walks, then per level: N, M, kind;  per dense body: n3}.
 *                  kind: 0 a level with a coarser one below, else how the last level is solved: 1 dense inverse (k_st_coarse_apply),
 *                  2 all sweeps in one workgroup (k_st_coarse), 3 one launch per sweep (k_st_spmv5).  Returns the number of values, < 0 if
 *                  cap is too small.  Level index l in tsl_mg_export = position in this list (l = 0 is the first stencil level).
 *   tsl_mg_export: array `what` of level `level` of hierarchy `hierarchy` to the host, exactly as the cycle reads it; cap = room in elements;
 *                  returns the number of elements, < 0 where the level has no such array.
 *                    TSL_MG_A      double[225 n]  slot-major: A[(s * 9 + e) * n + row], s = (dI + 2) * 5 + (dJ + 2)
 *                    TSL_MG_DINV   double[9 n]    row-major 3 x 3 per node;  level -1: the level-0 blocks, 9 * tot_NV, ORIGINAL vertex order
 *                    TSL_MG_OMEGA  double[2]      {omega, lambda};  level -1: level 0;  none on a dense last level
 *                    TSL_MG_ROWPOS int32[tot_NV]  level -1 only: the solver's row of every vertex (level 0 runs in that order: its power iteration starts
 *                                                 from a vector that is a function of the row)
 *                    TSL_MG_A32    float[225 n]   (levels with a coarser one below)
 *                    TSL_MG_S32    float[441 nc]  S[(s * 9 + e) * nc + crow], s = (dI + 3) * 7 + (dJ + 3)   (same levels)
 *                    TSL_MG_CINV   float[n3 * n3], TSL_MG_BAD int32[1]: dense last level and its bad-pivot flag
 *                    TSL_MG_BINV   float[n3 * ld], ld = n3 rounded up to 4, TSL_MG_BAD_BODY int32[1]: dense body `hierarchy` (level ignored)
 *   tsl_mg_apply:  z = M^-1 r, both 3 * tot_NV device vectors in the caller's vertex order: gather, then what one PCG iteration launches for
 *                  its preconditioner (mg_vcycle with the body sweep, or block Jacobi / body blocks with the multigrid off), scatter.
 *   tsl_solve_with: ONE solver of the hierarchy, no successor: method 0 pcg_restarts with the active preconditioner, 1 minres, 2 gmres,
 *                  3 bicgstab; cap <= 0: "cg_maxit".  stats->flag: 0 (method 0) / 1 (methods 1-3) when the solver met its own stopping rule,
 *                  3 otherwise; stats->method echoes the argument.  (hierarchy_fallback's rebuild of the preconditioner from the fully projected
 *                  assembly needs the state of a running time step: like tsl_solve, a call from outside a step runs behind the one in place.) */
enum { TSL_MG_A = 0, TSL_MG_DINV = 1, TSL_MG_OMEGA = 2, TSL_MG_A32 = 3, TSL_MG_S32 = 4, TSL_MG_CINV = 5, TSL_MG_BAD = 6, TSL_MG_BINV = 7, TSL_MG_BAD_BODY = 8, TSL_MG_ROWPOS = 9 };
int tsl_mg_info(tsl_ctx* ctx, int32_t* out_host, int32_t cap);
int tsl_mg_export(tsl_ctx* ctx, int32_t hierarchy, int32_t level, int32_t what, void* host, int64_t cap);
int tsl_mg_apply(tsl_ctx* ctx, const double* r_dev, double* z_dev);
int tsl_solve_with(tsl_ctx* ctx, int32_t method, int32_t cap, const double* rhs_dev, double* x_dev, tsl_solve_stats* stats_host);

/* ---- the operator of the Krylov solvers taken apart (tests/ only; csrc/op_test_api.hpp).  Like the hooks above they call the solver's own functions
 * and kernels and add no launch to any existing path.
 *   tsl_op_export: array `what` to the host as the next solve reads it; cap = room in elements; returns the number of elements (0 where a scene
 *                  without constraints has no such array).  int32: SLICE_OFF[n_slices + 1], SLICE_LEN[n_slices], COLIDX[n_slots], PERM, ROWPOS,
 *                  DIAG_PERM[tot_NV], CR_PTR[tot_NV + 1], CR_ENT[4 nc] ((constraint << 2) | slot), CR_ROWS[16 nc]; uint8: FZMASK[tot_NV]
 *                  (bit k: component k frozen, solver order); double: VALS / VALS_FULL[9 n_slots] (masked / unmasked, padded slots included),
 *                  MDT2[tot_NV], DINV / CDIAG[9 tot_NV] (solver order; formed first only if the context holds them to be stale).
 *   tsl_op_apply:  y = H x by one kernel, x and y 3 * tot_NV device vectors in the caller's vertex order.  kernel 0: k_spmv with the dot into slot 0 of
 *                  the scalar record (returned in *dot_host) plus k_contact_matvec; 1..7: variants 1..7 of tsl_bench_spmv (static matrix only, their
 *                  per-workgroup partials of x . y in part_host); 8: the plain product of the solvers (launch_spmv, contact rows folded in); 9: the
 *                  same kernel with partials, as MINRES launches it.  Returns the number of partials.
 *   tsl_pcg_trace: the start of a PCG run as the solver launches it and n_iter iterations with a threshold nothing meets, the ones behind the
 *                  first launched one by one (use_graph 0) or as replays of the captured chunk (1: n_iter - 1 must be a multiple of the chunk).
 *                  out_vec: x, r, z, p, the previous p, Ap (6 x 3 tot_NV, solver order); out_part: the partials of p.Ap, r.z, r.r (3 x cap_part,
 *                  counts in n_part[3]); out_scal[11]: rzh[0], rzh[1], thresh2, bb, rr_last, rz_last, pAp_last, flag, iters, n_part1, n_part2.
 *                  Returns the chunk. */
enum { TSL_OP_SLICE_OFF = 0, TSL_OP_SLICE_LEN = 1, TSL_OP_COLIDX = 2, TSL_OP_PERM = 3, TSL_OP_ROWPOS = 4, TSL_OP_DIAG_PERM = 5, TSL_OP_VALS = 6, TSL_OP_VALS_FULL = 7,
       TSL_OP_FZMASK = 8, TSL_OP_MDT2 = 9, TSL_OP_DINV = 10, TSL_OP_CDIAG = 11, TSL_OP_CR_PTR = 12, TSL_OP_CR_ENT = 13, TSL_OP_CR_ROWS = 14 };
int tsl_op_export(tsl_ctx* ctx, int32_t what, void* host, int64_t cap);
int tsl_op_apply(tsl_ctx* ctx, int32_t kernel, const double* x_dev, double* y_dev, double* dot_host, double* part_host, int32_t cap);
int tsl_pcg_trace(tsl_ctx* ctx, const double* rhs_dev, int32_t n_iter, int32_t use_graph, double* out_vec_host, double* out_part_host, int32_t cap_part, int32_t* n_part_host,
                  double* out_scal_host);

/* ---- scene groups: several scenes of ONE device whose sparse direct solves share their launches --------------------------------------------
 * The reference's trajectory-optimisation drivers roll out independent copies of one scene (training/trajopt_*.py, one rollout per candidate
 * trajectory); a single 100k-triangle scene leaves most of the chip idle during the latency-bound parts of its factorisation.  A group takes the
 * members' matrices, solution / right-hand side vectors and fronts into memory of its own, merges their plans, and tsl_group_step advances all
 * members by one time step in lock step: per member exactly tsl_step's kernels and decisions (BaseScene.time_step, BaseScene.py:1327-1370),
 * the factorisation and the first application of the factors as ONE set of launches for all.  A member's result is bit-identical to the one
 * tsl_step gives for it alone.  Members stay ordinary contexts: every other entry point (tsl_adjoint_step, tsl_solve, ...) works on them as before.
 *   tsl_group_create: ctxs[n] contexts of one device that use the sparse direct solve and belong to no group; destroying a member destroys the group.
 *   tsl_group_step:   pos / prev / vel / ref_angle[n] device pointers (as tsl_step), stats[n] host records (null: none).
 *   tsl_group_adjoint_step: Grad.transfer_grad (analytic_grad_single.py:217-257) of every member for the same reverse step -- the arguments of
 *                     tsl_adjoint_step as arrays of n, the n adjoint systems through one merged factorisation; same bits per member; stats[n] or null.
 *   tsl_group_info:   {plan merges, arena re-layouts, host seconds in merges, bytes of the group's arenas, merged factorisations, merged applications,
 *                     solves in which a member went on from the merged first pass on its own path (refinement, GMRES), dataflow launches of the merged
 *                     factorisations, merged factorisations redone on the block-step path after such a launch lost a flag}; nine values. */
typedef struct tsl_group tsl_group;
int tsl_group_create(tsl_ctx* const* ctxs, int32_t n, tsl_group** out);
void tsl_group_destroy(tsl_group* g);
int tsl_group_step(tsl_group* g, double* const* pos, double* const* prev_pos, double* const* vel, double* const* ref_angle, tsl_step_stats* stats_host);
int tsl_group_adjoint_step(tsl_group* g, int step, int T, const double* const* pos_buffer, double* const* pos_grad, const double* const* ref_buffer,
                           double* const* angleref_grad, double* const* tmp_z_frozen, const double* adj_damping_host, tsl_solve_stats* stats_host);
int tsl_group_info(tsl_group* g, double* out9_host);

#ifdef __cplusplus
}
#endif
#endif /* TSL_HIP_H */
