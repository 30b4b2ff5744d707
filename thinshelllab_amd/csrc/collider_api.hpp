// Host side of the half-space colliders inside libtsl_hip.so: the entry points tsl_set_colliders .. tsl_collider_grad of include/tsl_hip.h and, for
// the launch sites of tsl_hip.hip and adjoint_api.hpp, the kernel arguments and the launches of an assembly, an energy and a reverse step
// (k_collider.hpp).  Included by tsl_hip.hip behind its helpers (tsl_fail, TSL_TRY, HIP_OK, Scope, nblk), the way handle_api.hpp is;
// the list checks and the plane table are in collider_host.hpp, which has no device code.
#pragma once
#include "collider_host.hpp"
#include "k_collider.hpp"
#include "tsl_ctx.hpp"

// the collider kernels of an energy / assembly / reverse step run only while this holds: without it the launches are the ones they were
static bool colliders_on(const tsl_ctx* c) { return c->col.n > 0 && c->k_collider != 0.0; }
// the plane table as the scalars stand now
static ColliderPlanes collider_planes(const tsl_ctx* c) {
  ColliderPlanes P = c->col;
  P.k = c->k_collider; P.eps = c->eps_contact; P.eh = c->eps_v * c->dt;
  return P;
}
static ColliderArgs collider_args(const tsl_ctx* c) { return ColliderArgs{c->NV, c->col_mask.p}; }
static int collider_nblk(const tsl_ctx* c) { return nblk(c->NV, 256); }

// Colliders in an assembly: gradient rows and diagonal blocks behind the vertex terms on the same stream (nothing while no collider is on)
static void collider_assemble_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* grad) {
  if (!colliders_on(c)) return;
  hipLaunchKernelGGL(k_collider_assemble, dim3(collider_nblk(c)), dim3(256), 0, s, collider_planes(c), collider_args(c), pos, prev, (const int*)c->diag_blk.p, grad, c->vals_full.p);
}
static void collider_energy_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* e_part) {
  hipLaunchKernelGGL(k_collider_energy, dim3(collider_nblk(c)), dim3(256), 0, s, collider_planes(c), collider_args(c), pos, prev, e_part);
}
// the share of a reverse step that goes into pos_grad[s-1] (x_s, x_{s-1}, the adjoint solution p)
static void collider_backprop_launch(tsl_ctx* c, hipStream_t s, const double* x_s, const double* x_prev, const double* p, double* pg_prev) {
  if (!colliders_on(c)) return;
  hipLaunchKernelGGL(k_collider_backprop, dim3(collider_nblk(c)), dim3(256), 0, s, collider_planes(c), collider_args(c), (const int*)c->frozen.p, x_s, x_prev, p, pg_prev);
}

// The list is checked on the host (collider_host.hpp) and kept in the context; the mask is a device buffer of NV bytes.  A refusal leaves the
// previous list in place.  n = 0 removes the colliders.
extern "C" int tsl_set_colliders(tsl_ctx* c, const double* normals, const double* offsets, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  ColliderPlanes P = c->col;
  if (collider_validate(normals, offsets, mu, n, P, err)) return tsl_fail("tsl_set_colliders: %s", err.c_str());
  std::vector<uint8_t> mask;
  if (collider_mask_validate(c->NV, n, vertex_mask, mask, err)) return tsl_fail("tsl_set_colliders: %s", err.c_str());
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change)
  c->col.n = 0;
  if (n == 0) { c->col_mask.release(); c->col_part.release(); c->col_out.release(); return 0; }
  TSL_TRY(c->col_mask.upload(mask));
  TSL_TRY(c->col_part.alloc((size_t)COLLIDER_SLOTS * collider_nblk(c)));
  TSL_TRY(c->col_out.alloc(COLLIDER_SLOTS));
  c->col = P;
  return 0;
}
extern "C" int tsl_set_collider_offsets(tsl_ctx* c, const double* offsets) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->col.n == 0) return 0;
  std::string err;
  if (collider_offsets_validate(offsets, c->col, err)) return tsl_fail("tsl_set_collider_offsets: %s", err.c_str());
  return 0;
}
extern "C" int tsl_collider_count(tsl_ctx* c, int32_t* out) {
  if (!c || !out) return tsl_fail("tsl_collider_count: null argument");
  *out = c->col.n;
  return 0;
}
// read-outs, `per` values per collider: the partials joined in workgroup order, one copy to the host, one synchronisation
static int collider_readout(tsl_ctx* c, int per, double* out_host) {
  hipLaunchKernelGGL(k_collider_join, dim3(1), dim3(64), 0, c->stream, collider_nblk(c), (const double*)c->col_part.p, c->col_out.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, c->col_out.p, (size_t)per * c->col.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
// out_host (n x 3): the net force -sum_v g_v of every plane at the state (pos, prev_pos); k_collider = 0: zeros, no launch
extern "C" int tsl_collider_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  Scope scope(c);
  if (c->col.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("tsl_collider_force: null argument");
  if (c->k_collider == 0.0) { std::fill(out_host, out_host + 3 * (size_t)c->col.n, 0.0); return 0; }
  hipLaunchKernelGGL(k_collider_force, dim3(collider_nblk(c)), dim3(256), 0, c->stream, collider_planes(c), collider_args(c), pos, prev, c->col_part.p);
  return collider_readout(c, 3, out_host);
}
// out_host (n x 2): the share of one reverse step in d(loss)/d(o_j) and d(loss)/d(mu_j) at the tape state (pos = x_s, prev_pos = x_{s-1}) with the
// offsets of step s in place; p_dev null: the last adjoint solution
extern "C" int tsl_collider_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  Scope scope(c);
  if (c->col.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("tsl_collider_grad: null argument");
  if (c->k_collider == 0.0) { std::fill(out_host, out_host + 2 * (size_t)c->col.n, 0.0); return 0; }
  const double* p = p_dev ? p_dev : (const double*)c->pdir.p;
  hipLaunchKernelGGL(k_collider_grad, dim3(collider_nblk(c)), dim3(256), 0, c->stream, collider_planes(c), collider_args(c), (const int*)c->frozen.p, pos, prev, p, c->col_part.p);
  return collider_readout(c, 2, out_host);
}
