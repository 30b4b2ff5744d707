// Host side of the wind inside libtsl_hip.so (k_wind.hpp): the entry points tsl_set_wind .. tsl_wind_grad of include/tsl_hip.h and,
// for the launch sites of tsl_hip.hip and adjoint_api.hpp, the launches of an assembly, an energy and a reverse step.  Included by tsl_hip.hip behind
// handle_api.hpp (handle_pattern, and the helpers tsl_fail, TSL_TRY, HIP_OK, Scope, nblk); the list checks are in wind_host.hpp, which has no device
// code, the gather lists are handle_lists of handle_host.hpp.
#pragma once
#include "handle_host.hpp"
#include "k_wind.hpp"
#include "tsl_ctx.hpp"
#include "wind_host.hpp"

// the wind kernels of an energy / assembly / reverse step run only while this holds: without it the launches are the ones they were
static bool wind_on(const tsl_ctx* c) { return c->wind.n > 0 && c->wind.cn + c->wind.ct != 0.0; }
static WindArgs wind_args(const tsl_ctx* c) {
  const WindSet& S = c->wind;
  return WindArgs{S.n, S.cv.p, S.w.p, S.cn, S.ct, c->dt, S.W[0], S.W[1], S.W[2]};
}
static HandleLists_dev wind_lists_dev(const tsl_ctx* c) {
  const WindSet& S = c->wind;
  return HandleLists_dev{S.n_vert, S.n_blk, S.vl_v.p, S.vl_ptr.p, S.vl_ent.p, S.bl_addr.p, S.bl_ptr.p, S.bl_ent.p};
}
static int wind_nblk(const tsl_ctx* c) { return nblk(c->wind.n, 256); }

// The wind in an assembly: the face records, then the gradient rows (one lane per touched vertex) and the blocks (one lane per touched block), behind
// the colliders on the stream of the vertex terms (nothing while the wind is off)
static void wind_assemble_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* grad) {
  if (!wind_on(c)) return;
  const WindSet& S = c->wind;
  const HandleLists_dev L = wind_lists_dev(c);
  hipLaunchKernelGGL(k_wind_face, dim3(wind_nblk(c)), dim3(256), 0, s, wind_args(c), pos, prev, S.rec.p);
  if (grad) hipLaunchKernelGGL(k_wind_grad, dim3(nblk(L.n_vert, 256)), dim3(256), 0, s, S.n, L, (const double*)S.rec.p, grad);
  hipLaunchKernelGGL(k_wind_hess, dim3(nblk(L.n_blk, 256)), dim3(256), 0, s, S.n, 9.0 * c->dt, L, (const double*)S.rec.p, c->vals_full.p);
}
// Its energy partials from e_part on, one per workgroup of 256 faces; returns how many
static int wind_energy_launch(tsl_ctx* c, hipStream_t s, const double* pos, const double* prev, double* e_part) {
  if (!wind_on(c)) return 0;
  hipLaunchKernelGGL(k_wind_energy, dim3(wind_nblk(c)), dim3(256), 0, s, wind_args(c), pos, prev, e_part);
  return wind_nblk(c);
}
// Its share of a reverse step that goes into pos_grad[s-1] (x_s, x_{s-1}, the adjoint solution p): the lagged centroid and the lagged area vector
static void wind_backprop_launch(tsl_ctx* c, hipStream_t s, const double* x_s, const double* x_prev, const double* p, double* pg_prev) {
  if (!wind_on(c)) return;
  const WindSet& S = c->wind;
  const HandleLists_dev L = wind_lists_dev(c);
  hipLaunchKernelGGL(k_wind_backprop_face, dim3(wind_nblk(c)), dim3(256), 0, s, wind_args(c), (const int*)c->frozen.p, x_s, x_prev, p, S.stage.p);
  hipLaunchKernelGGL(k_wind_backprop, dim3(nblk(L.n_vert, 256)), dim3(256), 0, s, L, (const int*)c->frozen.p, (const double*)S.stage.p, pg_prev);
}

static void wind_release(tsl_ctx* c) {
  WindSet& S = c->wind;
  S.n = 0; S.n_vert = 0; S.n_blk = 0;
  S.cv.release(); S.w.release(); S.vl_v.release(); S.vl_ptr.release(); S.vl_ent.release(); S.bl_addr.release(); S.bl_ptr.release(); S.bl_ent.release();
  S.rec.release(); S.stage.release(); S.part.release(); S.out.release();
}
// The list is checked and its gather lists are built on the host; nothing of the previous list is touched before both have succeeded.  faces == NULL
// with n = -1: every cloth face in ascending order (weights, if given, one per cloth face).  n = 0 leaves no buffer behind.
extern "C" int tsl_set_wind(tsl_ctx* c, const int32_t* faces, const double* weights, int32_t n) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::vector<int32_t> all;
  if (!faces && n == -1) {
    all.resize((size_t)c->n_cface);
    for (int f = 0; f < c->n_cface; f++) all[f] = f;
    faces = all.data(); n = c->n_cface;
  }
  std::string err;
  if (wind_validate(c->n_cface, c->NF, faces, weights, n, err)) return tsl_fail("tsl_set_wind: %s", err.c_str());
  if (n > 0 && c->h_faces.size() < 3 * (size_t)c->NF) return tsl_fail("tsl_set_wind: the scene has no face table");
  std::vector<int> cv;
  HandleLists L;
  if (n > 0) {
    cv = handle_face_corners(c->h_faces.data(), faces, n);
    for (size_t e = 0; e < cv.size(); e++)
      if (cv[e] < 0 || cv[e] >= c->NV) return tsl_fail("tsl_set_wind: vertex %d of face %d (entry %d) out of range [0, %d)", cv[e], faces[e / 3], (int)(e / 3), c->NV);
    if (handle_lists(handle_pattern(c), cv.data(), n, 3, L, err, faces)) return tsl_fail("tsl_set_wind: %s", err.c_str());
  }
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change)
  wind_release(c);
  if (n == 0) return 0;
  WindSet& S = c->wind;
  std::vector<double> hw((size_t)n, 1.0);
  if (weights) hw.assign(weights, weights + n);
  TSL_TRY(S.cv.upload(cv));
  TSL_TRY(S.w.upload(hw));
  TSL_TRY(S.vl_v.upload(L.vl_v)); TSL_TRY(S.vl_ptr.upload(L.vl_ptr)); TSL_TRY(S.vl_ent.upload(L.vl_ent));
  TSL_TRY(S.bl_addr.upload(L.bl_addr)); TSL_TRY(S.bl_ptr.upload(L.bl_ptr)); TSL_TRY(S.bl_ent.upload(L.bl_ent));
  TSL_TRY(S.rec.alloc(9 * (size_t)n));
  TSL_TRY(S.stage.alloc(9 * (size_t)n));
  TSL_TRY(S.part.alloc(5 * (size_t)nblk(n, 256)));
  TSL_TRY(S.out.alloc(5));
  S.n_vert = (int)L.vl_v.size(); S.n_blk = (int)L.bl_addr.size();
  S.n = n;
  return 0;
}
// W (3 values, host) for the next energy, assemble, step or adjoint step; a non-finite component fails and leaves the velocity in place
extern "C" int tsl_set_wind_velocity(tsl_ctx* c, const double* W) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  if (wind_velocity_validate(W, c->wind.W, err)) return tsl_fail("tsl_set_wind_velocity: %s", err.c_str());
  return 0;
}
extern "C" int tsl_wind_count(tsl_ctx* c, int32_t* out) {
  if (!c || !out) return tsl_fail("tsl_wind_count: null argument");
  *out = c->wind.n;
  return 0;
}
// read-outs, N values: the partials joined in workgroup order, one copy to the host, one synchronisation; wind off: zeros, no launch
template <int N>
static int wind_readout(tsl_ctx* c, const char* who, const double* pos, const double* prev, const double* p, double* out_host) {
  Scope scope(c);
  if (!pos || !prev || !out_host) return tsl_fail("%s: null argument", who);
  if (!wind_on(c)) { std::fill(out_host, out_host + N, 0.0); return 0; }
  WindSet& S = c->wind;
  hipLaunchKernelGGL(k_wind_readout<N>, dim3(wind_nblk(c)), dim3(256), 0, c->stream, wind_args(c), (const int*)c->frozen.p, pos, prev, p, S.part.p);
  hipLaunchKernelGGL(k_wind_join, dim3(1), dim3(64), 0, c->stream, wind_nblk(c), N, (const double*)S.part.p, S.out.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, S.out.p, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
// out_host (3): the net force the wind applies to the cloth, -sum_f M_f r_f, at the state (pos, prev); frozen dofs are not masked
extern "C" int tsl_wind_force(tsl_ctx* c, const double* pos, const double* prev, double* out_host) {
  return wind_readout<3>(c, "tsl_wind_force", pos, prev, nullptr, out_host);
}
// out_host (5): the share of one reverse step in d(loss)/d(W, c_n, c_t) at the tape state (pos = x_s, prev = x_{s-1}) with the wind velocity of
// step s in place; p_dev null: the last adjoint solution
extern "C" int tsl_wind_grad(tsl_ctx* c, const double* pos, const double* prev, const double* p_dev, double* out_host) {
  return wind_readout<5>(c, "tsl_wind_grad", pos, prev, p_dev ? p_dev : (const double*)c->pdir.p, out_host);
}
