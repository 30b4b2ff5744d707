// Host side of the sphere colliders inside libtsl_hip.so: the entry points tsl_set_spheres .. tsl_sphere_grad of include/tsl_hip.h and, for the
// launch sites of tsl_hip.hip and adjoint_api.hpp, the kernel arguments and the launches of an assembly, an energy and a reverse step
// (k_sphere.hpp).  Included by tsl_hip.hip behind collider_api.hpp, the way that file is; the list checks and the table are in
// sphere_host.hpp, which has no device code.
#pragma once
#include "k_sphere.hpp"
#include "sphere_host.hpp"
#include "tsl_ctx.hpp"

// the sphere kernels of an energy / assembly / reverse step run only while this holds: without it the launches are the ones they were
static bool spheres_on(const tsl_ctx* c) { return c->sph.n > 0 && c->k_sphere != 0.0; }
// the table as the scalars stand now
static SphereTable sphere_table(const tsl_ctx* c) {
  SphereTable S = c->sph;
  S.k = c->k_sphere; S.eps = c->eps_contact; S.eh = c->eps_v * c->dt;
  return S;
}
static SphereArgs sphere_args(const tsl_ctx* c) { return SphereArgs{c->NV, c->sph_mask.p}; }
static int sphere_nblk(const tsl_ctx* c) { return nblk(c->NV, 256); }

// Spheres in an assembly: gradient rows and diagonal blocks behind the colliders on the same stream (nothing while no sphere is on).  spd 0: the
// exact block of the reverse step's operator; every other mode: the projected one
static void sphere_assemble_launch(tsl_ctx* c, hipStream_t s, int spd, const double* pos, const double* prev, double* grad) {
  if (!spheres_on(c)) return;
  hipLaunchKernelGGL(k_sphere_assemble, dim3(sphere_nblk(c)), dim3(256), 0, s, sphere_table(c), sphere_args(c), spd == 0 ? 1 : 0, pos, prev, (const int*)c->diag_blk.p, grad,
                     c->vals_full.p);
}
static void sphere_energy_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* e_part) {
  hipLaunchKernelGGL(k_sphere_energy, dim3(sphere_nblk(c)), dim3(256), 0, s, sphere_table(c), sphere_args(c), pos, prev, e_part);
}
// the share of a reverse step that goes into pos_grad[s-1] (x_s, x_{s-1}, the adjoint solution p)
static void sphere_backprop_launch(tsl_ctx* c, hipStream_t s, const double* x_s, const double* x_prev, const double* p, double* pg_prev) {
  if (!spheres_on(c)) return;
  hipLaunchKernelGGL(k_sphere_backprop, dim3(sphere_nblk(c)), dim3(256), 0, s, sphere_table(c), sphere_args(c), (const int*)c->frozen.p, x_s, x_prev, p, pg_prev);
}

// The list is checked on the host (sphere_host.hpp) and kept in the context; the mask is a device buffer of NV bytes.  A refusal leaves the
// previous list in place.  n = 0 removes the spheres.  The previous centres are the centres.
extern "C" int tsl_set_spheres(tsl_ctx* c, const double* centres, const double* radii, const double* mu, int32_t n, const uint8_t* vertex_mask) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  SphereTable S = c->sph;
  if (sphere_validate(centres, radii, mu, n, S, err)) return tsl_fail("tsl_set_spheres: %s", err.c_str());
  std::vector<uint8_t> mask;
  if (sphere_mask_validate(c->NV, n, vertex_mask, mask, err)) return tsl_fail("tsl_set_spheres: %s", err.c_str());
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change)
  c->sph.n = 0;
  if (n == 0) { c->sph_mask.release(); c->sph_part.release(); c->sph_out.release(); return 0; }
  TSL_TRY(c->sph_mask.upload(mask));
  TSL_TRY(c->sph_part.alloc((size_t)SPHERE_SLOTS * sphere_nblk(c)));
  TSL_TRY(c->sph_out.alloc(SPHERE_SLOTS));
  c->sph = S;
  return 0;
}
extern "C" int tsl_set_sphere_centres(tsl_ctx* c, const double* centres, const double* prev_centres) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->sph.n == 0) return 0;
  std::string err;
  if (sphere_centres_validate(centres, prev_centres, c->sph, err)) return tsl_fail("tsl_set_sphere_centres: %s", err.c_str());
  return 0;
}
extern "C" int tsl_sphere_count(tsl_ctx* c, int32_t* out) {
  if (!c || !out) return tsl_fail("tsl_sphere_count: null argument");
  *out = c->sph.n;
  return 0;
}
// read-outs, `per` values per sphere: the partials joined in workgroup order, one copy to the host, one synchronisation
static int sphere_readout(tsl_ctx* c, int per, double* out_host) {
  hipLaunchKernelGGL(k_sphere_join, dim3(1), dim3(64), 0, c->stream, sphere_nblk(c), c->sph.n, per, (const double*)c->sph_part.p, c->sph_out.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, c->sph_out.p, (size_t)per * c->sph.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
// out_host (n x 3): the net force -sum_v g_v of every ball at the state (pos, prev); k_sphere = 0: zeros, no launch
extern "C" int tsl_sphere_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  Scope scope(c);
  if (c->sph.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("tsl_sphere_force: null argument");
  if (c->k_sphere == 0.0) { std::fill(out_host, out_host + 3 * (size_t)c->sph.n, 0.0); return 0; }
  hipLaunchKernelGGL(k_sphere_force, dim3(sphere_nblk(c)), dim3(256), 0, c->stream, sphere_table(c), sphere_args(c), pos, prev, c->sph_part.p);
  return sphere_readout(c, 3, out_host);
}
// out_host (n x 8): the share of one reverse step in d(loss)/d(c_j, cp_j, mu_j, R_j) at the tape state (pos = x_s, prev = x_{s-1}) with the centres
// and previous centres of step s in place; p_dev null: the last adjoint solution
extern "C" int tsl_sphere_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  Scope scope(c);
  if (c->sph.n == 0) return 0;
  if (!pos || !prev || !out_host) return tsl_fail("tsl_sphere_grad: null argument");
  if (c->k_sphere == 0.0) { std::fill(out_host, out_host + 8 * (size_t)c->sph.n, 0.0); return 0; }
  const double* p = p_dev ? p_dev : (const double*)c->pdir.p;
  hipLaunchKernelGGL(k_sphere_grad, dim3(sphere_nblk(c)), dim3(256), 0, c->stream, sphere_table(c), sphere_args(c), (const int*)c->frozen.p, pos, prev, p, c->sph_part.p);
  return sphere_readout(c, 8, out_host);
}
