// Host side of the ties inside libtsl_hip.so: the entry points tsl_set_ties .. tsl_tie_count of include/tsl_hip.h (k_tie.hpp).
// Included by tsl_hip.hip behind its helpers (tsl_fail, TSL_TRY, HIP_OK, Scope, nblk), the way handle_api.hpp is; the list checks and the slot
// records are in tie_host.hpp, which has no device code; the slots are appended by contact_slots_finish (k_contact.hpp).
#pragma once
#include "k_tie.hpp"
#include "tie_host.hpp"
#include "tsl_ctx.hpp"

// a per-slot array with room for `count` entries; what it holds (the slots of the last detection) is kept
template <class T>
static int tie_grow(DevBuf<T>& b, size_t count) {
  if (b.n >= count) return 0;
  DevBuf<T> nb;
  TSL_TRY(nb.alloc(count));
  if (b.n) HIP_OK(hipMemcpy(nb.p, b.p, b.n * sizeof(T), hipMemcpyDeviceToDevice));
  b.swap(nb);
  return 0;
}
// every array that is sized by the number of constraint slots, for the scene's cap plus n ties (the scratch among them is allocated where it is used:
// c_G, c_H_pc and the row lists compare their size with contact_cap)
static int tie_reserve(tsl_ctx* c, size_t n) {
  const size_t mc = (size_t)c->max_n_constraints + n;
  if (c->c_idx.n >= 4 * mc) return 0;
  if (c->group) return tsl_fail("tsl_set_ties: the context is a member of a scene group, whose memory holds its constraint blocks: set the ties before the group is created");
  TSL_TRY(tie_grow(c->c_idx, mc * 4)); TSL_TRY(tie_grow(c->c_w, mc * 3)); TSL_TRY(tie_grow(c->c_n, mc * 3)); TSL_TRY(tie_grow(c->c_dx0, mc * 3));
  TSL_TRY(tie_grow(c->c_k, mc)); TSL_TRY(tie_grow(c->c_mu, mc)); TSL_TRY(tie_grow(c->c_T, mc * 6)); TSL_TRY(tie_grow(c->c_kind, mc));
  TSL_TRY(tie_grow(c->c_H, mc * 144)); TSL_TRY(tie_grow(c->c_Hfull, mc * 144));
  return 0;
}
// The tie slots as the list and k_tie stand now, behind the detected slots in place: the old tie slots leave, the new ones are appended and the row
// lists are built again (contact_slots_finish).  The factorisation plan compares the constraint set anew.
static int tie_slots_refresh(tsl_ctx* c) {
  c->nc -= c->nc_tie; c->nc_tie = 0;
  c->ds.cons_checked = false;
  c->bd_valid = false; c->cdiag_valid = false; c->dinv_valid = false;
  TSL_TRY(contact_slots_finish(c));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

// Ties: the list is checked and its records are built on the host (tie_host.hpp) and copied into buffers of the context.  A refusal leaves the
// previous list in place
extern "C" int tsl_set_ties(tsl_ctx* c, const int32_t* verts, const int32_t* faces, const double* bary, const double* weights, int32_t n) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  std::string err;
  if (tie_validate(c->NV, c->NF, c->h_faces.data(), verts, faces, bary, weights, n, err)) return tsl_fail("tsl_set_ties: %s", err.c_str());
  TSL_TRY(tie_reserve(c, (size_t)n));
  const TieRecords R = tie_records(c->h_faces.data(), verts, faces, bary, weights, n);
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // (the scale of the operator may change)
  c->nc -= c->nc_tie; c->nc_tie = 0; c->n_tie = 0;
  TSL_TRY(c->ti_idx.upload(R.idx)); TSL_TRY(c->ti_b.upload(R.b)); TSL_TRY(c->ti_w.upload(R.w));
  TSL_TRY(c->ti_out.alloc(3 * (size_t)n));
  c->n_tie = n;
  return tie_slots_refresh(c);
}
extern "C" int tsl_tie_count(tsl_ctx* c, int32_t* out) {
  if (!c || !out) return tsl_fail("tsl_tie_count: null argument");
  *out = c->n_tie;
  return 0;
}
// read-outs, `per` values per tie: the kernel writes ti_out, one copy to the host, one synchronisation
static int tie_readout(tsl_ctx* c, int per, double* out_host) {
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out_host, c->ti_out.p, (size_t)per * c->n_tie * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int tsl_tie_force(tsl_ctx* c, const double* pos, double* out_host) {
  Scope scope(c);
  if (c->n_tie == 0) return 0;
  if (!pos || !out_host) return tsl_fail("tsl_tie_force: null argument");
  hipLaunchKernelGGL(k_tie_force, dim3(nblk(c->n_tie, 256)), dim3(256), 0, c->stream, tie_args(c), pos, c->ti_out.p);
  return tie_readout(c, 3, out_host);
}
extern "C" int tsl_tie_residuals(tsl_ctx* c, const double* pos, double* out_host) {
  Scope scope(c);
  if (c->n_tie == 0) return 0;
  if (!pos || !out_host) return tsl_fail("tsl_tie_residuals: null argument");
  hipLaunchKernelGGL(k_tie_residual, dim3(nblk(c->n_tie, 256)), dim3(256), 0, c->stream, tie_args(c), pos, c->ti_out.p);
  return tie_readout(c, 3, out_host);
}
// out_host (n): k_tie g_i at the state pos, the contribution of one reverse step to d(loss)/d(w_i); p_dev null: the last adjoint solution
extern "C" int tsl_tie_grad(tsl_ctx* c, const double* pos, const double* p_dev, double* out_host) {
  Scope scope(c);
  if (c->n_tie == 0) return 0;
  if (!pos || !out_host) return tsl_fail("tsl_tie_grad: null argument");
  const double* p = p_dev ? p_dev : (const double*)c->pdir.p;
  hipLaunchKernelGGL(k_pg_tie, dim3(nblk(c->n_tie, PG_TIE_THREADS)), dim3(PG_TIE_THREADS), 0, c->stream, tie_args(c), pos, p, (const int*)c->frozen.p, c->ti_out.p, (double*)nullptr);
  return tie_readout(c, 1, out_host);
}
