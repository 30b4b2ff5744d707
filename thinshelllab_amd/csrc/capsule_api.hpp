// Host side of the capsule colliders inside libtsl_hip.so: the entry points tsl_set_capsules .. tsl_capsule_grad of include/tsl_hip.h and, for the
// launch sites of tsl_hip.hip and adjoint_api.hpp, the kernel arguments and the launches of an assembly, an energy and a reverse step
// (k_capsule.hpp).  Included by tsl_hip.hip behind sphere_api.hpp, the way that file is; the list checks and the table are in
// capsule_host.hpp, which has no device code.
#pragma once
#include "k_capsule.hpp"
#include "capsule_host.hpp"
#include "tsl_ctx.hpp"

// the capsule kernels of an energy / assembly / reverse step run only while this holds: without it the launches are the ones they were
static bool capsules_on(const tsl_ctx* c) { return c->cap.n > 0 && c->k_capsule != 0.0; }
// the table as the scalars stand now
static CapsuleTable capsule_table(const tsl_ctx* c) {
  CapsuleTable S = c->cap;
  S.k = c->k_capsule; S.eps = c->eps_contact; S.eh = c->eps_v * c->dt;
  return S;
}
static CapsuleArgs capsule_args(const tsl_ctx* c) { return CapsuleArgs{c->NV, c->cap_mask.p}; }
static int capsule_nblk(const tsl_ctx* c) { return nblk(c->NV, 256); }

// Capsules in an assembly: gradient rows and diagonal blocks behind the spheres on the same stream (nothing while no capsule is on).  spd 0: the
// exact block of the reverse step's operator; every other mode: the projected one
static void capsule_assemble_launch(tsl_ctx* c, hipStream_t s, int spd, const double* pos, const double* prev, double* grad) {
  if (!capsules_on(c)) return;
  hipLaunchKernelGGL(k_capsule_assemble, dim3(capsule_nblk(c)), dim3(256), 0, s, capsule_table(c), capsule_args(c), spd == 0 ? 1 : 0, pos, prev, (const int*)c->diag_blk.p, grad,
                     c->vals_full.p);
}
static void capsule_energy_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* e_part) {
  if (!capsules_on(c)) return;
  hipLaunchKernelGGL(k_capsule_energy, dim3(capsule_nblk(c)), dim3(256), 0, s, capsule_table(c), capsule_args(c), pos, prev, e_part);
}
// the share of a reverse step that goes into pos_grad[s-1] (x_s, x_{s-1}, the adjoint solution p)
static void capsule_backprop_launch(tsl_ctx* c, hipStream_t s, const double* x_s, const double* x_prev, const double* p, double* pg_prev) {
  if (!capsules_on(c)) return;
  hipLaunchKernelGGL(k_capsule_backprop, dim3(capsule_nblk(c)), dim3(256), 0, s, capsule_table(c), capsule_args(c), (const int*)c->frozen.p, x_s, x_prev, p, pg_prev);
}

// The list is checked on the host (capsule_host.hpp) and kept in the context; the mask is a device buffer of NV bytes.  A refusal leaves the
// previous list in place.  n = 0 removes the capsules.  The previous endpoints are the endpoints.
extern "C" int tsl_set_capsules(tsl_ctx* c, const double* a, const double* b, const double* radii, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  CapsuleTable S = c->cap;
  if (capsule_validate(a, b, radii, mu, n, S, err)) return tsl_fail("tsl_set_capsules: %s", err.c_str());
  std::vector<uint8_t> mask;
  if (capsule_mask_validate(c->NV, n, vertex_mask, mask, err)) return tsl_fail("tsl_set_capsules: %s", err.c_str());
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change)
  c->cap.n = 0;
  if (n == 0) { c->cap_mask.release(); c->cap_part.release(); c->cap_out.release(); return 0; }
  TSL_TRY(c->cap_mask.upload(mask));
  TSL_TRY(c->cap_part.alloc((size_t)CAPSULE_SLOTS * capsule_nblk(c)));
  TSL_TRY(c->cap_out.alloc(CAPSULE_SLOTS));
  c->cap = S;
  return 0;
}
extern "C" int tsl_set_capsule_ends(tsl_ctx* c, const double* a, const double* b, const double* prev_a, const double* prev_b) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->cap.n == 0) return 0;
  std::string err;
  if (capsule_ends_validate(a, b, prev_a, prev_b, c->cap, err)) return tsl_fail("tsl_set_capsule_ends: %s", err.c_str());
  return 0;
}
extern "C" int tsl_capsule_count(tsl_ctx* c, int32_t* out) {
  if (!c || !out) return tsl_fail("tsl_capsule_count: null argument");
  *out = c->cap.n;
  return 0;
}
// read-outs, `per` values per capsule: the partials joined in workgroup order, one copy to the host, one synchronisation
static int capsule_readout(tsl_ctx* c, int per, double* out_host) {
  hipLaunchKernelGGL(k_capsule_join, dim3(1), dim3(CAPSULE_SLOTS), 0, c->stream, capsule_nblk(c), c->cap.n, per, (const double*)c->cap_part.p, c->cap_out.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, c->cap_out.p, (size_t)per * c->cap.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
// out_host (n x 6): the net force -sum_v g_v of every rod and its torque -sum_v (x_v - m) x g_v about the rod's midpoint at the state (pos, prev);
// k_capsule = 0: zeros, no launch
extern "C" int tsl_capsule_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  Scope scope(c);
  if (c->cap.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("tsl_capsule_force: null argument");
  if (c->k_capsule == 0.0) { std::fill(out_host, out_host + 6 * (size_t)c->cap.n, 0.0); return 0; }
  hipLaunchKernelGGL(k_capsule_force, dim3(capsule_nblk(c)), dim3(256), 0, c->stream, capsule_table(c), capsule_args(c), pos, prev, c->cap_part.p);
  return capsule_readout(c, 6, out_host);
}
// out_host (n x 14): the share of one reverse step in d(loss)/d(a_j, b_j, ap_j, bp_j, mu_j, R_j) at the tape state (pos = x_s, prev = x_{s-1}) with the
// endpoints and previous endpoints of step s in place; p_dev null: the last adjoint solution
extern "C" int tsl_capsule_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  Scope scope(c);
  if (c->cap.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("tsl_capsule_grad: null argument");
  if (c->k_capsule == 0.0) { std::fill(out_host, out_host + 14 * (size_t)c->cap.n, 0.0); return 0; }
  const double* p = p_dev ? p_dev : (const double*)c->pdir.p;
  hipLaunchKernelGGL(k_capsule_grad, dim3(capsule_nblk(c)), dim3(256), 0, c->stream, capsule_table(c), capsule_args(c), (const int*)c->frozen.p, pos, prev, p, c->cap_part.p);
  return capsule_readout(c, 14, out_host);
}
