// The reverse step, Grad.transfer_grad (analytic_grad_single.py:217-257) without the gripper part (host: gripper.set / gather_grad), in two halves
// around the linear solve p = H^-1 pos_grad[s] (tsl_adjoint_step: the scene's own solve; tsl_group_adjoint_step: the merged solve of a scene group).
// Included by tsl_hip.hip behind the solves.
#pragma once
#include "k_adjoint.hpp"

struct AdjArgs { int step, T; const double* pos_buffer; double* pos_grad; const double* ref_buffer; double* angleref_grad; double* tmp_z_frozen; double adj_damping; };

// What one reverse step reads and writes on the tape: rows s, s - 1 and s - 2 (null at step 1) of pos_grad, rows s and s - 1 of pos_buffer and
// angleref_grad, row s - 1 of ref_buffer; n3, nr: doubles per row of the positions / of the rest angles.  Built once per step, read by both halves
struct AdjStep { size_t n3, nr; double *pg_s, *pg_prev, *pg_prev2; const double *x_s, *x_prev; double *ag_s, *ag_prev; const double* ref_prev; double* tmp_z_frozen; double adj_damping; };
static AdjStep adj_step(const tsl_ctx* c, const AdjArgs& a) {
  AdjStep t;
  t.n3 = 3 * (size_t)c->NV; t.nr = 3 * (size_t)std::max(c->n_cface, 1);
  const size_t s = (size_t)a.step;
  t.pg_s = a.pos_grad + s * t.n3; t.pg_prev = a.pos_grad + (s - 1) * t.n3; t.pg_prev2 = s > 1 ? a.pos_grad + (s - 2) * t.n3 : nullptr;
  t.x_s = a.pos_buffer + s * t.n3; t.x_prev = a.pos_buffer + (s - 1) * t.n3;
  t.ag_s = a.angleref_grad + s * t.nr; t.ag_prev = a.angleref_grad + (s - 1) * t.nr; t.ref_prev = a.ref_buffer + (s - 1) * t.nr;
  t.tmp_z_frozen = a.tmp_z_frozen; t.adj_damping = a.adj_damping;
  return t;
}

// clamp, contacts at x_{s-1}, ref-angle backprop (a2ax), the un-projected Hessian at x_s in c->vals / c->c_H; the right-hand side is t.pg_s
static int adjoint_pre(tsl_ctx* c, const AdjStep& t) {
  hipStream_t s = c->stream;
  // clamp_grad
  hipLaunchKernelGGL(k_clamp, dim3(gsz(t.n3)), dim3(256), 0, s, t.n3, t.pg_s, c->adj_clamp);
  if (c->n_cface && c->adj_clamp_angleref)
    hipLaunchKernelGGL(k_clamp, dim3(gsz(3 * (size_t)c->n_cface)), dim3(256), 0, s, 3 * (size_t)c->n_cface, t.ag_s, 1000.0);
  // contacts re-detected at pos = prev_pos = x_{s-1} (copy_pos_only + calc_vn + f_contact + contact_analysis)
  int nc = 0;
  if (c->contact_enable) TSL_TRY(tsl_contact_detect(c, t.x_prev, t.x_prev, &nc));
  else TSL_TRY(contact_slots_none(c));
  ClothArgs CA = cloth_args(c);
  TSL_TRY(ensure_vg_stage(c));
  // pos = x_s, ref_angle = ref_{s-1}: init_folding + ref_angle_backprop_a2ax
  if (c->n_hinge) {
    CA.gstage = c->vg_stage.p;
    hipLaunchKernelGGL(k_adj_a2ax, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, CA, t.x_s, t.ref_prev, t.ag_s, t.ag_prev);
    vertex_gather_launch(c, s, c->vg_stage.p, c->vg_hinge0, c->vg_tet0, t.pg_s);
    CA.gstage = nullptr;
  }
  // preconditioner from the SPD-projected Hessian of the same state (block Jacobi + multigrid hierarchy): the operator
  // below is the un-projected H, which may be indefinite, and smoothers / coarse operators built from it are not safe
  const bool have_mg = !c->mg.empty() && c->mg_enable != 0;
  // the direct path factorises the un-projected operator itself; its auto mode may still probe the hierarchy first (not marked hard)
  const bool spd_pc = c->adj_spd_pc && (have_mg || body_active(c)) && !(direct_enabled(c) && (c->ds.enable == 1 || c->ds.hard || c->n_tet > 0 || c->nc > 0));   // (no probe of the hierarchy: see solve_direct)
  c->bd_valid = false;
  c->mg_omega_valid = false;
  if (spd_pc) {
    TSL_TRY(assemble(c, t.x_s, t.x_prev, t.x_prev, t.ref_prev, 1, nullptr));
    if (body_active(c)) TSL_TRY(body_build_inverse(c));
    if (have_mg) TSL_TRY(mg_setup_operators(c));
    if (c->vals_pc.n == 0 && c->vals_pc.alloc(c->vals.n)) return tsl_fail("out of device memory (vals_pc)");
    HIP_OK(hipMemcpyAsync(c->vals_pc.p, c->vals.p, c->vals.n * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (c->nc > 0) {
      if (c->c_H_pc.n < c->c_H.n && c->c_H_pc.alloc(c->c_H.n)) return tsl_fail("out of device memory (c_H_pc)");
      HIP_OK(hipMemcpyAsync(c->c_H_pc.p, c->c_H.p, (size_t)c->nc * 144 * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    c->pc_frozen = true;
  }
  // H.clear_all + compute_Hessian(False)
  const int rc_asm = assemble(c, t.x_s, t.x_prev, t.x_prev /*vel unused without gradient*/, t.ref_prev, 0, nullptr);
  c->pc_frozen = false;
  if (rc_asm) return rc_asm;
  if (spd_pc) c->pc_separate = true;
  return 0;
}

// p = c->pdir (original order), c->v_x (permuted): tmp_z_frozen, contact / ref-angle / inertia backprop into step s-1 and s-2
static int adjoint_post(tsl_ctx* c, const AdjStep& t) {
  hipStream_t s = c->stream;
  const int NV = c->NV;
  ClothArgs CA = cloth_args(c);
  // tmp_z_frozen (second compute_Hessian pass with counting_z_frozen)
  hipLaunchKernelGGL(k_zfrozen_gather, dim3(nblk(NV, 256)), dim3(256), 0, s, NV, c->slice_off.p, c->slice_len.p, c->colidx.p, (const int*)c->trans.p, c->fzmask.p, c->vals_full.p,
                     c->v_x.p, c->v_t4.p);
  hipLaunchKernelGGL(k_scatter_perm, dim3(nblk(NV, 256)), dim3(256), 0, s, NV, c->perm.p, c->v_t4.p, t.tmp_z_frozen);
  if (c->nc > 0) {
    hipLaunchKernelGGL(k_contact_zfrozen_gather, dim3(nblk((long)NV * 64, 256)), dim3(256), 0, s, NV, (const int*)c->rowpos.p, (const int*)c->cr_ptr.p, (const int*)c->cr_ent.p, c->c_idx.p,
                       c->frozen.p, c->c_Hfull.p, c->pdir.p, t.tmp_z_frozen);
  }
  // contact_energy_backprop(step-1) ; ref_angle_backprop_x2a
  // (a tie's energy depends on the current positions only: it carries nothing into the earlier steps.  Its rows of c_G are cleared, so that the
  // row gather adds zeros for them and not what the last assembly left there)
  if (c->nc > c->nc_tie) {
    if (c->c_G.n < 12 * contact_cap(c)) { if (c->c_G.alloc(12 * contact_cap(c))) return -1; }
    const int nvf = contact_nvf(c);
    if (c->nc_tie > 0) HIP_OK(hipMemsetAsync(c->c_G.p + 12 * (size_t)(c->nc - c->nc_tie), 0, 12 * (size_t)c->nc_tie * sizeof(double), s));
    if (nvf > 0) hipLaunchKernelGGL(k_contact_backprop, dim3(nblk(nvf, 64)), dim3(64), 0, s, nvf, contact_args(c), t.x_s, c->pdir.p, c->c_G.p);
    if (c->nc_ee > 0) hipLaunchKernelGGL(k_ee_backprop, dim3(nblk(c->nc_ee, 64)), dim3(64), 0, s, c->nc_ee, ee_args(contact_args(c), nvf), t.x_s, c->pdir.p, c->c_G.p + 12 * (size_t)nvf);
    hipLaunchKernelGGL(k_contact_row_gather, dim3(nblk((long)NV * 64, 256)), dim3(256), 0, s, NV, (const int*)c->rowpos.p, (const int*)c->cr_ptr.p, (const int*)c->cr_ent.p,
                       (const double*)c->c_G.p, t.pg_prev);
  }
  if (c->n_hinge) hipLaunchKernelGGL(k_adj_x2a, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, CA, t.x_s, c->pdir.p, t.ag_prev);
  // the colliders' lagged terms (planes, balls, rods): -(dg / dx_prev)^T p into the vertices' own rows of pos_grad[s-1] (nothing while none is on)
  shapes_backprop_launch(c, s, t.x_s, t.x_prev, c->pdir.p, t.pg_prev);
  // the wind's lagged terms: the lagged centroid and the lagged area vector of every listed face, into the rows of its corners (nothing while it is off)
  wind_backprop_launch(c, s, t.x_s, t.x_prev, c->pdir.p, t.pg_prev);
  // get_prev_grad / get_prev_prev_grad
  hipLaunchKernelGGL(k_adj_prev, dim3(gsz(t.n3)), dim3(256), 0, s, NV, c->pdir.p, c->mass.p, c->frozen.p, c->dt, t.adj_damping, t.pg_prev, t.pg_prev2);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int tsl_adjoint_step(tsl_ctx* c, int step, int T, const double* pos_buffer, double* pos_grad, const double* ref_buffer, double* angleref_grad,
                                double* tmp_z_frozen, double adj_damping, tsl_solve_stats* st) {
  Scope scope(c);
  if (step < 1 || step >= T) return tsl_fail("tsl_adjoint_step: step %d outside [1, %d)", step, T);
  const AdjStep t = adj_step(c, AdjArgs{step, T, pos_buffer, pos_grad, ref_buffer, angleref_grad, tmp_z_frozen, adj_damping});
  TSL_TRY(adjoint_pre(c, t));
  // p = H^-1 pos_grad[s]
  tsl_solve_stats local;
  if (!st) st = &local;
  TSL_TRY(solve_orig(c, t.pg_s, c->pdir.p, st));
  if (st->method == 4) TSL_TRY(direct_prezero(c));   // the next adjoint step assembles another operator
  if (c->verbose) fprintf(stderr, "[tsl] adjoint step %d: nc %d solver flag %d iters %d restarts %d rel_residual %.2e\n", step, c->nc, st->flag, st->iters, st->restarts, st->rel_residual);
  TSL_TRY(adjoint_post(c, t));
  HIP_OK(hipStreamSynchronize(c->stream));
  HIP_OK(hipGetLastError());
  return 0;
}

// Grad.transfer_grad of every scene of a group for the same reverse step: the S adjoint systems H_i p_i = pos_grad_i[s] go through ONE merged
// factorisation and first application (group_solve), the halves before and after it run per member on its own stream (one host thread each).
// Same bits per scene as tsl_adjoint_step on a context with the sparse direct solve.  stats: S records (or NULL).
extern "C" int tsl_group_adjoint_step(tsl_group* G, int step, int T, const double* const* pos_buffer_a, double* const* pos_grad_a, const double* const* ref_buffer_a,
                                      double* const* angleref_grad_a, double* const* tmp_z_a, const double* adj_damping_a, tsl_solve_stats* stats) {
  const int n = (int)G->m.size();
  tsl_ctx* g = G->g;
  if (step < 1 || step >= T) return tsl_fail("tsl_group_adjoint_step: step %d outside [1, %d)", step, T);
  std::vector<std::unique_ptr<Scope>> scopes;
  for (int i = 0; i < n; i++) scopes.emplace_back(new Scope(G->m[i]));
  std::vector<AdjStep> tt(n);
  std::vector<int> act(n);
  for (int i = 0; i < n; i++) {
    if (!direct_enabled(G->m[i])) return tsl_fail("tsl_group_adjoint_step: scene %d does not use the sparse direct solve", i);
    tt[i] = adj_step(G->m[i], AdjArgs{step, T, pos_buffer_a[i], pos_grad_a[i], ref_buffer_a[i], angleref_grad_a[i], tmp_z_a[i], adj_damping_a[i]});
    act[i] = i;
  }
  g->verbose = G->m[0]->verbose;
  TSL_TRY(G->pool->run(act, [&](int i) -> int {
    tsl_ctx* c = G->m[i];
    TSL_TRY(adjoint_pre(c, tt[i]));
    hipLaunchKernelGGL(k_gather_perm, dim3(nblk(c->NV, 256)), dim3(256), 0, c->stream, c->NV, c->perm.p, (const double*)tt[i].pg_s, c->v_b.p);
    return 0;
  }));
  std::vector<tsl_solve_stats> ss;
  TSL_TRY(group_solve(G, act, ss, [](int) {}));
  TSL_TRY(G->pool->run(act, [&](int i) -> int {
    tsl_ctx* c = G->m[i];
    hipLaunchKernelGGL(k_scatter_perm, dim3(nblk(c->NV, 256)), dim3(256), 0, c->stream, c->NV, c->perm.p, (const double*)c->v_x.p, c->pdir.p);
    if (c->verbose) fprintf(stderr, "[tsl] group adjoint step %d, scene %d: nc %d solver flag %d iters %d restarts %d rel_residual %.2e\n", step, i, c->nc, ss[i].flag, ss[i].iters, ss[i].restarts,
                            ss[i].rel_residual);
    TSL_TRY(adjoint_post(c, tt[i]));
    return 0;
  }));
  for (int i = 0; i < n; i++) {
    HIP_OK(hipStreamSynchronize(G->m[i]->stream));
    if (stats) stats[i] = ss[i];
  }
  HIP_OK(hipGetLastError());
  return 0;
}
