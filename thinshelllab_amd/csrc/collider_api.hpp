// Host side of the five collider kinds inside libtsl_hip.so -- planes (k_collider.hpp), balls (k_sphere.hpp; 2.9), rods (k_capsule.hpp;
// 2.10), rounded boxes (k_box.hpp; 2.12), sampled distance fields (k_sdf.hpp; 2.14): the entry points tsl_set_colliders .. tsl_sdf_grad of include/tsl_hip.h and, for the launch sites of tsl_hip.hip and adjoint_api.hpp,
// the launches of an assembly, an energy and a reverse step.  One set of helpers, templates on the kind's Shape (k_shape.hpp);
// an entry point checks what is particular to its kind (collider_host.hpp, sphere_host.hpp, capsule_host.hpp, box_host.hpp, sdf_host.hpp) and hands on.  Included by
// tsl_hip.hip behind its helpers (tsl_fail, TSL_TRY, HIP_OK, Scope, nblk), the way handle_api.hpp is.
#pragma once
#include <type_traits>
#include "k_box.hpp"
#include "k_capsule.hpp"
#include "k_collider.hpp"
#include "k_sdf.hpp"
#include "k_sphere.hpp"
#include "tsl_ctx.hpp"

template <class Shape>
static auto& shape_set(tsl_ctx* c) {
  if constexpr (std::is_same_v<Shape, PlaneShape>) return c->col;
  else if constexpr (std::is_same_v<Shape, SphereShape>) return c->sph;
  else if constexpr (std::is_same_v<Shape, CapsuleShape>) return c->cap;
  else if constexpr (std::is_same_v<Shape, BoxShape>) return c->box;
  else return c->sdf;
}
// the kernels of a kind in an energy / assembly / reverse step run only while this holds: without it the launches are the ones they were
template <class Shape>
static bool shape_on(tsl_ctx* c) { return shape_set<Shape>(c).tab.n > 0 && shape_set<Shape>(c).k != 0.0; }
// the table as the scalars stand now
template <class Shape>
static typename Shape::Table shape_table(tsl_ctx* c) {
  typename Shape::Table T = shape_set<Shape>(c).tab;
  T.k = shape_set<Shape>(c).k; T.eps = c->eps_contact; T.eh = c->eps_v * c->dt;
  return T;
}
template <class Shape>
static ShapeArgs shape_args(tsl_ctx* c) { return ShapeArgs{c->NV, shape_set<Shape>(c).mask.p}; }
static int shape_nblk(const tsl_ctx* c) { return nblk(c->NV, 256); }
// how many kinds hold shapes, on or not (they size the energy partials)
static int shapes_present(tsl_ctx* c) { return (c->col.tab.n > 0) + (c->sph.tab.n > 0) + (c->cap.tab.n > 0) + (c->box.tab.n > 0) + (c->sdf.tab.n > 0); }

template <class Shape>
static void shape_assemble_launch(tsl_ctx* c, hipStream_t s, int spd, const double* pos, const double* prev, double* grad) {
  if (!shape_on<Shape>(c)) return;
  hipLaunchKernelGGL(k_shape_assemble<Shape>, dim3(shape_nblk(c)), dim3(256), 0, s, shape_table<Shape>(c), shape_args<Shape>(c), spd == 0 ? 1 : 0, pos, prev,
                     (const int*)c->diag_blk.p, grad, c->vals_full.p);
}
template <class Shape>
static void shape_energy_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* e_part, int& nb) {
  if (!shape_on<Shape>(c)) return;
  hipLaunchKernelGGL(k_shape_energy<Shape>, dim3(shape_nblk(c)), dim3(256), 0, s, shape_table<Shape>(c), shape_args<Shape>(c), pos, prev, e_part + nb);
  nb += shape_nblk(c);
}
template <class Shape>
static void shape_backprop_launch(tsl_ctx* c, hipStream_t s, const double* x_s, const double* x_prev, const double* p, double* pg_prev) {
  if (!shape_on<Shape>(c)) return;
  hipLaunchKernelGGL(k_shape_backprop<Shape>, dim3(shape_nblk(c)), dim3(256), 0, s, shape_table<Shape>(c), shape_args<Shape>(c), (const int*)c->frozen.p, x_s, x_prev, p, pg_prev);
}

// The colliders in an assembly: gradient rows and diagonal blocks behind the vertex terms on the same stream -- planes, then balls, then rods, then boxes, then fields; a
// kind that is not on launches nothing.  spd 0: the exact block of the reverse step's operator; every other mode: the projected one
static void shapes_assemble_launch(tsl_ctx* c, hipStream_t s, int spd, const double* pos, const double* prev, double* grad) {
  shape_assemble_launch<PlaneShape>(c, s, spd, pos, prev, grad);
  shape_assemble_launch<SphereShape>(c, s, spd, pos, prev, grad);
  shape_assemble_launch<CapsuleShape>(c, s, spd, pos, prev, grad);
  shape_assemble_launch<BoxShape>(c, s, spd, pos, prev, grad);
  shape_assemble_launch<SdfShape>(c, s, spd, pos, prev, grad);
}
// Their energy partials from e_part on, one per workgroup of 256 vertices and kind that is on, in the same order; returns how many
static int shapes_energy_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* e_part) {
  int nb = 0;
  shape_energy_launch<PlaneShape>(c, s, pos, prev, e_part, nb);
  shape_energy_launch<SphereShape>(c, s, pos, prev, e_part, nb);
  shape_energy_launch<CapsuleShape>(c, s, pos, prev, e_part, nb);
  shape_energy_launch<BoxShape>(c, s, pos, prev, e_part, nb);
  shape_energy_launch<SdfShape>(c, s, pos, prev, e_part, nb);
  return nb;
}
// Their share of a reverse step that goes into pos_grad[s-1] (x_s, x_{s-1}, the adjoint solution p), in the same order: the planes' lagged
// friction; the balls' lagged friction and lagged contact frame; the rods' lagged friction, lagged contact frame and lagged rod parameter; the boxes' lagged friction, lagged contact frame and lagged material point; the fields' likewise
static void shapes_backprop_launch(tsl_ctx* c, hipStream_t s, const double* x_s, const double* x_prev, const double* p, double* pg_prev) {
  shape_backprop_launch<PlaneShape>(c, s, x_s, x_prev, p, pg_prev);
  shape_backprop_launch<SphereShape>(c, s, x_s, x_prev, p, pg_prev);
  shape_backprop_launch<CapsuleShape>(c, s, x_s, x_prev, p, pg_prev);
  shape_backprop_launch<BoxShape>(c, s, x_s, x_prev, p, pg_prev);
  shape_backprop_launch<SdfShape>(c, s, x_s, x_prev, p, pg_prev);
}

// The tail of tsl_set_*: T is the checked list of n shapes (the kind's host header); the mask is checked here and becomes a device buffer of NV
// bytes.  A refusal leaves the previous list in place.  n = 0 removes the kind.
template <class Shape>
static int shape_commit(tsl_ctx* c, const char* who, const char* noun, const typename Shape::Table& T, int32_t n, const uint8_t* vertex_mask) {
  auto& S = shape_set<Shape>(c);
  std::string err;
  std::vector<uint8_t> mask;
  if (shape_mask_validate(noun, c->NV, n, vertex_mask, mask, err)) return tsl_fail("%s: %s", who, err.c_str());
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change)
  S.tab.n = 0;
  if (n == 0) { S.mask.release(); S.part.release(); S.out.release(); return 0; }
  TSL_TRY(S.mask.upload(mask));
  TSL_TRY(S.part.alloc((size_t)(SHAPE_MAX * Shape::stride) * shape_nblk(c)));
  TSL_TRY(S.out.alloc(SHAPE_MAX * Shape::stride));
  S.tab = T;
  return 0;
}
template <class Shape>
static int shape_count(tsl_ctx* c, const char* who, int32_t* out) {
  if (!c || !out) return tsl_fail("%s: null argument", who);
  *out = shape_set<Shape>(c).tab.n;
  return 0;
}
// read-outs, `per` values per shape: the partials joined in workgroup order, one copy to the host, one synchronisation
template <class Shape>
static int shape_readout(tsl_ctx* c, int per, double* out_host) {
  auto& S = shape_set<Shape>(c);
  hipLaunchKernelGGL(k_shape_join, dim3(1), dim3(SHAPE_MAX * Shape::stride), 0, c->stream, shape_nblk(c), S.tab.n, per, Shape::stride, (const double*)S.part.p, S.out.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, S.out.p, (size_t)per * S.tab.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
// out_host (n x Shape::n_force) at the state (pos, prev); no shape: nothing; stiffness 0: zeros, no launch
template <class Shape>
static int shape_force(tsl_ctx* c, const char* who, const double* pos, const double* prev, double* out_host) {
  Scope scope(c);
  auto& S = shape_set<Shape>(c);
  if (S.tab.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("%s: null argument", who);
  if (S.k == 0.0) { std::fill(out_host, out_host + Shape::n_force * (size_t)S.tab.n, 0.0); return 0; }
  hipLaunchKernelGGL(k_shape_force<Shape>, dim3(shape_nblk(c)), dim3(256), 0, c->stream, shape_table<Shape>(c), shape_args<Shape>(c), pos, prev, S.part.p);
  return shape_readout<Shape>(c, Shape::n_force, out_host);
}
// out_host (n x Shape::n_grad): the share of one reverse step at the tape state (pos = x_s, prev = x_{s-1}) with the table of step s in place;
// p_dev null: the last adjoint solution
template <class Shape>
static int shape_grad(tsl_ctx* c, const char* who, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  Scope scope(c);
  auto& S = shape_set<Shape>(c);
  if (S.tab.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("%s: null argument", who);
  if (S.k == 0.0) { std::fill(out_host, out_host + Shape::n_grad * (size_t)S.tab.n, 0.0); return 0; }
  const double* p = p_dev ? p_dev : (const double*)c->pdir.p;
  hipLaunchKernelGGL(k_shape_grad<Shape>, dim3(shape_nblk(c)), dim3(256), 0, c->stream, shape_table<Shape>(c), shape_args<Shape>(c), (const int*)c->frozen.p, pos, prev, p, S.part.p);
  return shape_readout<Shape>(c, Shape::n_grad, out_host);
}

// ---- planes.  Force: n x 3, the net force -sum_v g_v of every plane.  Grad: n x 2, d(loss)/d(o_j) and d(loss)/d(mu_j), the offsets of step s in place
extern "C" int tsl_set_colliders(tsl_ctx* c, const double* normals, const double* offsets, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  ColliderPlanes P = c->col.tab;
  if (collider_validate(normals, offsets, mu, n, P, err)) return tsl_fail("tsl_set_colliders: %s", err.c_str());
  return shape_commit<PlaneShape>(c, "tsl_set_colliders", "collider", P, n, vertex_mask);
}
extern "C" int tsl_set_collider_offsets(tsl_ctx* c, const double* offsets) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->col.tab.n == 0) return 0;
  std::string err;
  if (collider_offsets_validate(offsets, c->col.tab, err)) return tsl_fail("tsl_set_collider_offsets: %s", err.c_str());
  return 0;
}
extern "C" int tsl_collider_count(tsl_ctx* c, int32_t* out) { return shape_count<PlaneShape>(c, "tsl_collider_count", out); }
extern "C" int tsl_collider_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  return shape_force<PlaneShape>(c, "tsl_collider_force", pos, prev, out_host);
}
extern "C" int tsl_collider_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  return shape_grad<PlaneShape>(c, "tsl_collider_grad", pos, prev, p_dev, out_host);
}

// ---- balls.  The previous centres of a new list are its centres.  Force: n x 3, the net force -sum_v g_v of every ball.  Grad: n x 8,
// d(loss)/d(c_j, cp_j, mu_j, R_j), the centres and previous centres of step s in place
extern "C" int tsl_set_spheres(tsl_ctx* c, const double* centres, const double* radii, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  SphereTable S = c->sph.tab;
  if (sphere_validate(centres, radii, mu, n, S, err)) return tsl_fail("tsl_set_spheres: %s", err.c_str());
  return shape_commit<SphereShape>(c, "tsl_set_spheres", "sphere", S, n, vertex_mask);
}
extern "C" int tsl_set_sphere_centres(tsl_ctx* c, const double* centres, const double* prev_centres) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->sph.tab.n == 0) return 0;
  std::string err;
  if (sphere_centres_validate(centres, prev_centres, c->sph.tab, err)) return tsl_fail("tsl_set_sphere_centres: %s", err.c_str());
  return 0;
}
extern "C" int tsl_sphere_count(tsl_ctx* c, int32_t* out) { return shape_count<SphereShape>(c, "tsl_sphere_count", out); }
extern "C" int tsl_sphere_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  return shape_force<SphereShape>(c, "tsl_sphere_force", pos, prev, out_host);
}
extern "C" int tsl_sphere_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  return shape_grad<SphereShape>(c, "tsl_sphere_grad", pos, prev, p_dev, out_host);
}

// ---- rods.  The previous endpoints of a new list are its endpoints.  Force: n x 6, the net force -sum_v g_v of every rod and its torque
// -sum_v (x_v - m) x g_v about the rod's midpoint.  Grad: n x 14, d(loss)/d(a_j, b_j, ap_j, bp_j, mu_j, R_j), the endpoints and previous endpoints of
// step s in place
extern "C" int tsl_set_capsules(tsl_ctx* c, const double* a, const double* b, const double* radii, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  CapsuleTable S = c->cap.tab;
  if (capsule_validate(a, b, radii, mu, n, S, err)) return tsl_fail("tsl_set_capsules: %s", err.c_str());
  return shape_commit<CapsuleShape>(c, "tsl_set_capsules", "capsule", S, n, vertex_mask);
}
extern "C" int tsl_set_capsule_ends(tsl_ctx* c, const double* a, const double* b, const double* prev_a, const double* prev_b) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->cap.tab.n == 0) return 0;
  std::string err;
  if (capsule_ends_validate(a, b, prev_a, prev_b, c->cap.tab, err)) return tsl_fail("tsl_set_capsule_ends: %s", err.c_str());
  return 0;
}
extern "C" int tsl_capsule_count(tsl_ctx* c, int32_t* out) { return shape_count<CapsuleShape>(c, "tsl_capsule_count", out); }
extern "C" int tsl_capsule_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  return shape_force<CapsuleShape>(c, "tsl_capsule_force", pos, prev, out_host);
}
extern "C" int tsl_capsule_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  return shape_grad<CapsuleShape>(c, "tsl_capsule_grad", pos, prev, p_dev, out_host);
}

// ---- rounded boxes.  The previous poses of a new list are its poses.  Force: n x 6, the net force -sum_v g_v of every box and its torque
// -sum_v (x_v - c) x g_v about the box's centre.  Grad: n x 14, d(loss)/d(c_j, theta_j, cp_j, theta_p_j, mu_j, r_j), the poses and previous poses of
// step s in place
extern "C" int tsl_set_boxes(tsl_ctx* c, const double* centres, const double* quats, const double* half_extents, const double* radii, const double* mu, int32_t n,
                             const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  BoxTable S = c->box.tab;
  if (box_validate(centres, quats, half_extents, radii, mu, n, S, err)) return tsl_fail("tsl_set_boxes: %s", err.c_str());
  return shape_commit<BoxShape>(c, "tsl_set_boxes", "box", S, n, vertex_mask);
}
extern "C" int tsl_set_box_poses(tsl_ctx* c, const double* centres, const double* quats, const double* prev_centres, const double* prev_quats) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->box.tab.n == 0) return 0;
  std::string err;
  if (box_poses_validate(centres, quats, prev_centres, prev_quats, c->box.tab, err)) return tsl_fail("tsl_set_box_poses: %s", err.c_str());
  return 0;
}
extern "C" int tsl_box_count(tsl_ctx* c, int32_t* out) { return shape_count<BoxShape>(c, "tsl_box_count", out); }
extern "C" int tsl_box_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  return shape_force<BoxShape>(c, "tsl_box_force", pos, prev, out_host);
}
extern "C" int tsl_box_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  return shape_grad<BoxShape>(c, "tsl_box_grad", pos, prev, p_dev, out_host);
}

// ---- sampled distance fields.  The previous poses of a new list are its poses.  The samples of all fields go into one device buffer: a new list is
// checked, uploaded into a NEW buffer and swapped in once everything succeeded, so that a refusal leaves the previous list and the previous samples in
// place; n = 0 (and the context's destruction) frees the buffer.  Force: n x 6, the net force -sum_v g_v of every field and its torque
// -sum_v (x_v - c) x g_v about the field's centre.  Grad: n x 14, d(loss)/d(c_j, theta_j, cp_j, theta_p_j, mu_j, r_j), the poses and previous poses of
// step s in place
extern "C" int tsl_set_sdfs(tsl_ctx* c, const double* samples, const int32_t* dims, const double* origins, const double* spacings, const double* centres, const double* quats,
                            const double* offsets, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  SdfTable S = c->sdf.tab;
  size_t total = 0;
  if (sdf_validate(samples, dims, origins, spacings, centres, quats, offsets, mu, n, S, total, err)) return tsl_fail("tsl_set_sdfs: %s", err.c_str());
  DevBuf<double> fresh;
  if (n > 0) {
    TSL_TRY(fresh.alloc(total));
    HIP_OK(hipMemcpy(fresh.p, samples, total * sizeof(double), hipMemcpyHostToDevice));
  }
  S.smp = fresh.p;
  TSL_TRY(shape_commit<SdfShape>(c, "tsl_set_sdfs", "field", S, n, vertex_mask));
  c->sdf_smp.swap(fresh);   // (the previous buffer leaves with `fresh`)
  return 0;
}
extern "C" int tsl_set_sdf_poses(tsl_ctx* c, const double* centres, const double* quats, const double* prev_centres, const double* prev_quats) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->sdf.tab.n == 0) return 0;
  std::string err;
  if (sdf_poses_validate(centres, quats, prev_centres, prev_quats, c->sdf.tab, err)) return tsl_fail("tsl_set_sdf_poses: %s", err.c_str());
  return 0;
}
extern "C" int tsl_sdf_count(tsl_ctx* c, int32_t* out) { return shape_count<SdfShape>(c, "tsl_sdf_count", out); }
extern "C" int tsl_sdf_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  return shape_force<SdfShape>(c, "tsl_sdf_force", pos, prev, out_host);
}
extern "C" int tsl_sdf_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  return shape_grad<SdfShape>(c, "tsl_sdf_grad", pos, prev, p_dev, out_host);
}
