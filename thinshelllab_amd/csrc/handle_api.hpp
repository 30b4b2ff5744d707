// Host side of the soft handles and their rigid frames inside libtsl_hip.so: the entry points tsl_set_handles .. tsl_frame_grad of include/tsl_hip.h
// and, for the launch sites of tsl_hip.hip, the kernel arguments, handle_dispatch and the launches of an assembly (k_handle.hpp, k_frame.hpp;
// DESIGN.md 2.4 - 2.6).  Included by tsl_hip.hip behind its helpers (tsl_fail, TSL_TRY, HIP_OK, Scope, nblk), the way direct_host.hpp is; the list checks and the gather lists are in
// handle_host.hpp and frame_host.hpp, which have no device code.
#pragma once
#include <type_traits>

#include "frame_host.hpp"
#include "handle_host.hpp"
#include "k_frame.hpp"
#include "k_handle.hpp"
#include "tsl_ctx.hpp"

static HandleArgs handle_args(tsl_ctx* c) { return HandleArgs{c->n_handle, c->hd_cv.p, c->hd_cb.p, c->hd_w.p, c->hd_t.p, c->k_handle}; }
static HandleLists_dev handle_lists_dev(tsl_ctx* c) {
  return HandleLists_dev{c->n_hd_vert, c->n_hd_blk, c->hd_vl_v.p, c->hd_vl_ptr.p, c->hd_vl_ent.p, c->hd_bl_addr.p, c->hd_bl_ptr.p, c->hd_bl_ent.p};
}
// the handle kernels of an energy / assembly / reverse step run only while this holds: without it the launches are the ones they were
static bool handles_on(const tsl_ctx* c) { return c->n_handle > 0 && c->k_handle != 0.0; }
// The handle kernels are templates on the corners per handle: launch(NC) is called with NC a compile-time 1 (a vertex list) or 3 (a face list), as
// the list in place has it.  The one place where the kind of the list is looked at.
template <class Launch>
static void handle_dispatch(const tsl_ctx* c, Launch&& launch) {
  if (c->hd_nc == 1) launch(std::integral_constant<int, 1>());
  else launch(std::integral_constant<int, 3>());
}

// Soft handles in an assembly: their gradient rows (one lane per touched vertex) and block diagonals (one lane per touched block) behind the vertex
// terms on the same stream (nothing while no handle is on)
static void handle_assemble_launch(tsl_ctx* c, hipStream_t s, const double* pos, double* grad) {
  if (!handles_on(c)) return;
  const HandleArgs A = handle_args(c);
  const HandleLists_dev L = handle_lists_dev(c);
  handle_dispatch(c, [&](auto NC) {
    if (grad) hipLaunchKernelGGL(k_handle_grad<NC>, dim3(nblk(L.n_vert, 256)), dim3(256), 0, s, A, L, pos, grad);
    hipLaunchKernelGGL(k_handle_hess<NC>, dim3(nblk(L.n_blk, 256)), dim3(256), 0, s, A, L, c->vals_full.p);
  });
}

// Rigid frames of the handles (k_frame.hpp)
static void frames_release(tsl_ctx* c) {
  c->n_frame = 0;
  c->fr_of.release(); c->fr_ptr.release(); c->fr_idx.release(); c->fr_local.release(); c->fr_c.release(); c->fr_R.release(); c->fr_out.release();
}
static FrameArgs frame_args(tsl_ctx* c) { return FrameArgs{c->n_frame, c->fr_of.p, c->fr_local.p, c->fr_c.p, c->fr_R.p, c->fr_ptr.p, c->fr_idx.p}; }
// the framed rows of the target buffer from the poses as they stand (nothing without frames); the caller synchronises
static void frame_targets_launch(tsl_ctx* c) {
  if (c->n_frame == 0 || c->n_handle == 0) return;
  hipLaunchKernelGGL(k_frame_targets, dim3(nblk(c->n_handle, 256)), dim3(256), 0, c->stream, c->n_handle, frame_args(c), c->hd_t.p);
}

// The tail of both setters.  The list is checked and, for n > 0, its gather lists L are built from its corners cv (n x nc; cb: their coordinates,
// none for nc = 1); nothing of the previous list has been touched before.  The new list replaces it and the frames (they went with the list they
// numbered); n = 0 leaves no buffer behind.  Targets start at zero.
static int handles_upload(tsl_ctx* c, int nc, int32_t n, const std::vector<int>& cv, const std::vector<double>& cb, const double* weights, const HandleLists& L) {
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change: |H|_inf is formed again when a refinement asks for it)
  c->n_handle = 0;
  frames_release(c);
  std::vector<double> hw((size_t)n, 1.0);
  if (weights) hw.assign(weights, weights + n);
  TSL_TRY(c->hd_cv.upload(cv));
  TSL_TRY(c->hd_cb.upload(cb));
  TSL_TRY(c->hd_vl_v.upload(L.vl_v)); TSL_TRY(c->hd_vl_ptr.upload(L.vl_ptr)); TSL_TRY(c->hd_vl_ent.upload(L.vl_ent));
  TSL_TRY(c->hd_bl_addr.upload(L.bl_addr)); TSL_TRY(c->hd_bl_ptr.upload(L.bl_ptr)); TSL_TRY(c->hd_bl_ent.upload(L.bl_ent));
  TSL_TRY(c->hd_w.upload(hw));
  TSL_TRY(c->hd_t.upload(std::vector<double>(3 * (size_t)n, 0.0)));
  TSL_TRY(c->hd_out.alloc(3 * (size_t)n));
  c->n_hd_vert = (int)L.vl_v.size(); c->n_hd_blk = (int)L.bl_addr.size();
  c->hd_nc = nc;
  c->n_handle = n;
  return 0;
}
// the pattern the context keeps, as Pattern::lookup reads it: the rows, their positions and the slice offsets
static Pattern handle_pattern(const tsl_ctx* c) {
  Pattern P;
  P.rows = c->h_rows; P.rowpos = c->h_rowpos; P.slice_off = c->h_slice_off;
  return P;
}
// Handles on vertices: the list is checked and the gather lists are built on the host (handle_host.hpp) and copied into buffers of the context
extern "C" int tsl_set_handles(tsl_ctx* c, const int32_t* verts, const double* weights, int32_t n) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  if (handle_validate(c->NV, verts, weights, n, err)) return tsl_fail("tsl_set_handles: %s", err.c_str());
  const std::vector<int> cv(verts, verts + (n > 0 ? n : 0));
  HandleLists L;
  if (n > 0 && handle_lists(handle_pattern(c), cv.data(), n, 1, L, err)) return tsl_fail("tsl_set_handles: %s", err.c_str());
  return handles_upload(c, 1, n, cv, {}, weights, L);
}
// Handles at barycentric points of faces: the corners are the vertices of the faces in the scene's global face table; conventions of tsl_set_handles
extern "C" int tsl_set_handles_on_faces(tsl_ctx* c, const int32_t* faces, const double* bary, const double* weights, int32_t n) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  if (handle_face_validate(c->NV, c->NF, c->h_faces.data(), faces, bary, weights, n, err)) return tsl_fail("tsl_set_handles_on_faces: %s", err.c_str());
  const std::vector<int> cv = handle_face_corners(c->h_faces.data(), faces, n);
  HandleLists L;
  if (n > 0 && handle_lists(handle_pattern(c), cv.data(), n, 3, L, err, faces)) return tsl_fail("tsl_set_handles_on_faces: %s", err.c_str());
  return handles_upload(c, 3, n, cv, std::vector<double>(bary, bary + 3 * (size_t)n), weights, L);
}
extern "C" int tsl_set_handle_targets(tsl_ctx* c, const double* targets) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->n_handle == 0) return 0;
  if (!targets) return tsl_fail("tsl_set_handle_targets: null targets for %d handles", c->n_handle);
  HIP_OK(hipMemcpy(c->hd_t.p, targets, 3 * (size_t)c->n_handle * sizeof(double), hipMemcpyHostToDevice));
  if (c->n_frame > 0) {   // the rows of framed handles follow their frame, whichever of the targets and the poses was set last
    frame_targets_launch(c);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(c->stream));
  }
  return 0;
}
// read-outs, one value per handle and axis: the kernel writes hd_out, one copy to the host, one synchronisation
static int handle_readout(tsl_ctx* c, double* out_host) {
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, c->hd_out.p, 3 * (size_t)c->n_handle * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int tsl_handle_force(tsl_ctx* c, const double* pos, double* out_host) {
  Scope scope(c);
  if (c->n_handle == 0) return 0;
  if (!pos || !out_host) return tsl_fail("tsl_handle_force: null argument");
  handle_dispatch(c, [&](auto NC) { hipLaunchKernelGGL(k_handle_force<NC>, dim3(nblk(c->n_handle, 256)), dim3(256), 0, c->stream, handle_args(c), pos, c->hd_out.p); });
  return handle_readout(c, out_host);
}
extern "C" int tsl_handle_points(tsl_ctx* c, const double* pos, double* out_host) {
  Scope scope(c);
  if (c->n_handle == 0) return 0;
  if (!pos || !out_host) return tsl_fail("tsl_handle_points: null argument");
  handle_dispatch(c, [&](auto NC) { hipLaunchKernelGGL(k_handle_points<NC>, dim3(nblk(c->n_handle, 256)), dim3(256), 0, c->stream, handle_args(c), pos, c->hd_out.p); });
  return handle_readout(c, out_host);
}
extern "C" int tsl_handle_grad(tsl_ctx* c, const double* p_dev, double* out_host) {
  Scope scope(c);
  if (c->n_handle == 0) return 0;
  if (!out_host) return tsl_fail("tsl_handle_grad: null argument");
  const double* p = p_dev ? p_dev : (const double*)c->pdir.p;
  handle_dispatch(c, [&](auto NC) { hipLaunchKernelGGL(k_handle_backprop<NC>, dim3(nblk(c->n_handle, 256)), dim3(256), 0, c->stream, handle_args(c), p, (const int*)c->frozen.p, c->hd_out.p); });
  return handle_readout(c, out_host);
}

// Rigid frames for the handles (k_frame.hpp): lists checked and the CSR built on the host (frame_host.hpp), copies the context owns; conventions of
// tsl_set_handles.  Poses start at the identity at the origin
extern "C" int tsl_set_handle_frames(tsl_ctx* c, const int32_t* frame_of, const double* local, int32_t n_frame) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  if (frame_validate(c->n_handle, frame_of, local, n_frame, err)) return tsl_fail("tsl_set_handle_frames: %s", err.c_str());
  frames_release(c);
  if (n_frame == 0) return 0;
  const size_t n = (size_t)c->n_handle;
  std::vector<int> ptr, idx;
  frame_csr(c->n_handle, frame_of, n_frame, ptr, idx);
  std::vector<double> hl(local, local + 3 * n), hR(9 * (size_t)n_frame, 0.0);
  for (size_t i = 0; i < n; i++)
    if (frame_of[i] < 0) hl[3 * i] = hl[3 * i + 1] = hl[3 * i + 2] = 0.0;   // (never read; keeps what is uploaded finite)
  for (int j = 0; j < n_frame; j++) hR[9 * (size_t)j] = hR[9 * (size_t)j + 4] = hR[9 * (size_t)j + 8] = 1.0;
  TSL_TRY(c->fr_of.upload(std::vector<int>(frame_of, frame_of + n)));
  TSL_TRY(c->fr_local.upload(hl));
  TSL_TRY(c->fr_ptr.upload(ptr));
  TSL_TRY(c->fr_idx.upload(idx));
  TSL_TRY(c->fr_c.upload(std::vector<double>(3 * (size_t)n_frame, 0.0)));
  TSL_TRY(c->fr_R.upload(hR));
  TSL_TRY(c->fr_out.alloc(6 * (size_t)n_frame));
  c->n_frame = n_frame;
  frame_targets_launch(c);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int tsl_set_frame_poses(tsl_ctx* c, const double* pos, const double* quat) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->n_frame == 0) return 0;
  std::string err;
  std::vector<double> hc, hR;
  if (frame_pose_matrices(pos, quat, c->n_frame, hc, hR, err)) return tsl_fail("tsl_set_frame_poses: %s", err.c_str());
  HIP_OK(hipMemcpy(c->fr_c.p, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(c->fr_R.p, hR.data(), hR.size() * sizeof(double), hipMemcpyHostToDevice));
  frame_targets_launch(c);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int tsl_handle_targets(tsl_ctx* c, double* out_host) {
  Scope scope(c);
  if (c->n_handle == 0) return 0;
  if (!out_host) return tsl_fail("tsl_handle_targets: null argument");
  HIP_OK(hipMemcpyAsync(out_host, c->hd_t.p, 3 * (size_t)c->n_handle * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
// read-outs, six values per frame: one workgroup per frame writes fr_out, one copy to the host, one synchronisation; k_handle = 0: zeros, no launch
template <int MODE>
static int frame_readout(tsl_ctx* c, const double* vec, double* out_host) {
  if (c->k_handle == 0.0) { std::fill(out_host, out_host + 6 * (size_t)c->n_frame, 0.0); return 0; }
  handle_dispatch(c, [&](auto NC) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_frame_reduce<MODE, NC>), dim3(c->n_frame), dim3(256), 0, c->stream, handle_args(c), frame_args(c), vec, (const int*)c->frozen.p, c->fr_out.p); });
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, c->fr_out.p, 6 * (size_t)c->n_frame * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int tsl_frame_wrench(tsl_ctx* c, const double* pos, double* out_host) {
  Scope scope(c);
  if (c->n_frame == 0) return 0;
  if (!pos || !out_host) return tsl_fail("tsl_frame_wrench: null argument");
  return frame_readout<FRAME_WRENCH>(c, pos, out_host);
}
extern "C" int tsl_frame_grad(tsl_ctx* c, const double* p_dev, double* out_host) {
  Scope scope(c);
  if (c->n_frame == 0) return 0;
  if (!out_host) return tsl_fail("tsl_frame_grad: null argument");
  return frame_readout<FRAME_GRAD>(c, p_dev ? p_dev : (const double*)c->pdir.p, out_host);
}
