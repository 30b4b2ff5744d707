// Read-outs of a state or of the last reverse step, the entry points of system identification: the internal force of the bodies, and the
// gradients of the loss in the friction coefficient, in the reference's {kb, mu, lam} and in any differentiated key (table, key resolution and
// partial layout: param_keys.hpp; passes: k_param.hpp).  Included by tsl_hip.hip behind the assembly helpers.
#pragma once

// ------------------------------------------------------------------------------------------------
// Internal force field of the FEM bodies (Elastic.get_force): consumed by BaseScene.check_early_stop / gather_force
// (BaseScene.py:1541-1584).  force_dev: tot_NV x 3 (only the rows of elastic bodies are written, the rest is zeroed).
extern "C" int tsl_elastic_force(tsl_ctx* c, const double* pos, double* force) {
  Scope scope(c);
  hipStream_t s = c->stream;
  const size_t n3 = 3 * (size_t)c->NV;
  HIP_OK(hipMemsetAsync(force, 0, n3 * sizeof(double), s));
  if (c->n_tet) {
    TetArgs TA = tet_args(c);
    // element gradients staged and summed per vertex in a fixed order (as in the assembly)
    TSL_TRY(ensure_vg_stage(c));
    TA.gstage = c->vg_stage.p + 3 * (size_t)c->vg_tet0;
    hipLaunchKernelGGL(k_tet_grad, dim3(nblk(c->n_tet, 256)), dim3(256), 0, s, TA, pos);
    vertex_gather_launch(c, s, c->vg_stage.p, c->vg_tet0, c->vg_ns, force);
    for (const ElasticDev& e : c->h_el)
      hipLaunchKernelGGL(k_elastic_force_finish, dim3(nblk(e.n_verts, 256)), dim3(256), 0, s, vert_args(c), e.v_offset, e.v_offset + e.n_verts, force);
  }
  HIP_OK(hipStreamSynchronize(s));
  HIP_OK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Friction-coefficient gradient of the system-identification adjoint (Scene_sliding.contact_energy_backprop_friction,
// Scene_sliding.py:139-176; called from analytic_grad_system.transfer_grad :150-151 instead of get_parameters_grad):
// contribution of the last tsl_adjoint_step to d(loss)/d(mu_cloth_cloth).  pos = tape state x_s.
extern "C" int tsl_friction_grad(tsl_ctx* c, const double* pos, double* out_host) {
  Scope scope(c);
  hipStream_t s = c->stream;
  const int nvf = contact_nvf(c);
  if (c->nc_ee > 0) {   // edge-edge slots of the mu_cloth_cloth pairs: no gradient (restating the vertex-triangle term with the edge-edge weights disagreed with
                        // differences in mu by orders of magnitude), so the call fails instead of returning a wrong number
    std::vector<int> kind(c->nc_ee);
    HIP_OK(hipMemcpyAsync(kind.data(), c->c_kind.p + nvf, kind.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (int k : kind)
      if (k == 2) return tsl_fail("tsl_friction_grad: %d edge-edge constraints (contact_ee = 1) use mu_cloth_cloth; their friction-coefficient gradient is not implemented", c->nc_ee);
  }
  double* acc = &SC(c)->aux[0];
  HIP_OK(hipMemsetAsync(acc, 0, sizeof(double), s));
  if (nvf > 0)
    hipLaunchKernelGGL(k_contact_friction_grad, dim3(nblk(nvf, 64)), dim3(64), 0, s, nvf, contact_args(c), c->c_kind.p, c->frozen.p, pos, c->pdir.p, c->mu_cloth_cloth, acc,
                       nblk(nvf, 64) <= 64 * 512 ? c->dot_part.p : (double*)nullptr, c->dot_ticket.p);

  HIP_OK(hipMemcpyAsync(out_host, acc, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Parameter gradients of the system-identification adjoint (analytic_grad_system.py:69-80 with BaseScene.get_paramters_grad
// :1513-1525, Cloth.compute_deri model_fold_offset.py:1082-1127, Elastic.compute_deri): sum over the free dofs of
// p . d(force)/d(parameter), p = the solution of the last tsl_adjoint_step.  out = {kb, mu, lam}; lam is always 0
// because the reference never pushes d_lam up to the scene.
extern "C" int tsl_param_grad(tsl_ctx* c, const double* pos, const double* ref, double* out_host) {
  Scope scope(c);
  hipStream_t s = c->stream;
  const int NV = c->NV;
  const size_t n3 = 3 * (size_t)NV;
  double* tmp = c->v_t4.p;
  double* acc = &SC(c)->aux[0];
  HIP_OK(hipMemsetAsync(acc, 0, 2 * sizeof(double), s));
  // hinge / tet contributions staged per element and summed per vertex in a fixed order, the dot products joined from per-block partials -- two runs of a
  // system-identification sweep give the same bits
  TSL_TRY(ensure_vg_stage(c));
  // d_kb = -(bending gradient) / Kb per cloth
  if (c->n_hinge) {
    HIP_OK(hipMemsetAsync(tmp, 0, n3 * sizeof(double), s));
    hipLaunchKernelGGL(k_cloth_normals, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, c->n_cface, pos, c->cf_f2v.p, c->norm_dir.p);
    ClothArgs CA = cloth_args(c);
    CA.gstage = c->vg_stage.p;
    hipLaunchKernelGGL(k_cloth_grad_hinge, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, CA, pos, ref);
    vertex_gather_launch(c, s, c->vg_stage.p, c->vg_hinge0, c->vg_tet0, tmp);
    for (const ClothDev& cd : c->h_cloth)
      hipLaunchKernelGGL(k_dot_free, dim3(DOT_BLOCKS), dim3(256), 0, s, 3 * (size_t)cd.v_offset, 3 * (size_t)(cd.v_offset + cd.NV), c->pdir.p, tmp, c->frozen.p, -1.0 / cd.Kb, acc, DOT_SCRATCH(c));
  }
  // d_mu
  if (c->n_tet) {
    if (c->dmu_accum.n == 0) { TSL_TRY(c->dmu_accum.alloc(n3)); HIP_OK(hipMemsetAsync(c->dmu_accum.p, 0, n3 * sizeof(double), s)); }
    HIP_OK(hipMemsetAsync(tmp, 0, n3 * sizeof(double), s));
    if (c->vg_stage2.n < 12 * (size_t)c->n_tet) { if (c->vg_stage2.alloc(12 * (size_t)c->n_tet)) return tsl_fail("out of device memory (gradient staging)"); }
    double *stA = c->vg_stage.p + 3 * (size_t)c->vg_tet0, *stB = c->vg_stage2.p;
    hipLaunchKernelGGL(k_tet_deri_mu, dim3(nblk(c->n_tet, 64)), dim3(64), 0, s, tet_args(c), pos, stA, stB);
    {   // (the second gather reads the same slot numbers from a staging array that holds the tet slots only)
      vertex_gather_launch(c, s, c->vg_stage.p, c->vg_tet0, c->vg_ns, tmp);
      vertex_gather_launch(c, s, c->vg_stage2.p - 3 * (size_t)c->vg_tet0, c->vg_tet0, c->vg_ns, c->dmu_accum.p);
    }
    hipLaunchKernelGGL(k_dot_free, dim3(DOT_BLOCKS), dim3(256), 0, s, (size_t)0, n3, c->pdir.p, tmp, c->frozen.p, 1.0, acc + 1, DOT_SCRATCH(c));
    hipLaunchKernelGGL(k_dot_free, dim3(DOT_BLOCKS), dim3(256), 0, s, (size_t)0, n3, c->pdir.p, c->dmu_accum.p, c->frozen.p, 1.0, acc + 1, DOT_SCRATCH(c));
  }
  double h[2];
  HIP_OK(hipMemcpyAsync(h, acc, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  out_host[0] = h[0]; out_host[1] = h[1]; out_host[2] = 0.0;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Parameter gradients by key (system identification beyond the reference's {kb, mu, lam}): out[j] = -sum over the free dofs of p . dF/d(theta_j),
// F = the gradient of tsl_assemble at (pos, ref_angle) with the contact constraints as they stand -- the sign of tsl_param_grad, whose kb is the sum
// of the cloth<i>.Kb values.  One pass per element class that some requested key needs (k_param.hpp), each writing one partial per workgroup and key
// row; k_pg_final sums the requested keys' partials; one read-back.
extern "C" int tsl_param_grad_keys(tsl_ctx* c, const double* pos, const double* ref, const double* p_dev, const char* const* keys, int32_t n_keys,
                                   double* out_host) {
  Scope scope(c);
  if (n_keys <= 0) return 0;
  if (!keys || !out_host || !pos) return tsl_fail("tsl_param_grad_keys: null argument");
  hipStream_t s = c->stream;
  const int n_cloth = (int)c->h_cloth.size(), n_el = (int)c->h_el.size();
  const int nvf = contact_nvf(c);
  // ---- keys -> (class, row), and what a key asks of the live state
  std::vector<PgRow> kr(n_keys);
  bool need[PG_NCLASS] = {};
  std::string err;
  std::vector<int> tie_keys;   // "k_tie" is resolved ahead of the table (tie_host.hpp): its partials lie behind the table's, so no row of the table moves
  for (int j = 0; j < n_keys; j++) {
    if (!keys[j]) return tsl_fail("tsl_param_grad_keys: key %d is null", j);
    if (!strcmp(keys[j], PG_TIE_KEY)) { tie_keys.push_back(j); kr[j] = PgRow{PG_HANDLE, 0}; continue; }   // (a placeholder row: its table entry is rewritten below)
    if (pg_resolve_key(keys[j], n_cloth, n_el, kr[j], err)) return tsl_fail("%s", err.c_str());
    const int row = kr[j].row;
    if (kr[j].cls == PG_CONTACT) {
      if (row == PG_ROW_K_CONTACT && c->nc_ee > 0)
        return tsl_fail("tsl_param_grad_keys: k_contact: %d edge-edge constraints (contact_ee = 1) are present; their friction derivative is not implemented", c->nc_ee);
      const double live = row == PG_ROW_K_CONTACT ? c->k_contact : (row == PG_ROW_MU_CLOTH_ELASTIC ? c->mu_cloth_elastic : c->mu_cloth_cloth);
      bool used = row == PG_ROW_K_CONTACT;
      for (const auto& pr : c->h_pairs) used |= pr.mu_is_param == row;   // (mu_is_param 1 / 2: the pair's mu is the live mu_cloth_elastic / mu_cloth_cloth)
      if (live == 0.0 && used && nvf > 0)
        return tsl_fail("tsl_param_grad_keys: %s = 0: the friction weights c_k of the detection vanish with it, their derivative is not available", keys[j]);
    }
    if (kr[j].cls == PG_HINGE && !ref) return tsl_fail("tsl_param_grad_keys: %s needs ref_angle", keys[j]);
    need[kr[j].cls] = true;
  }
  // ---- partial layout: one partial per row and workgroup of a needed class.  With no cloth of membrane = 1 the StVK keys have no partials and read
  //      exact zeros, as k_handle does with no handles
  auto groups = [](int n) { return n > 0 ? nblk(n, PG_THREADS) : 0; };
  int nb[PG_NCLASS];
  nb[PG_FACE] = groups(c->n_cface); nb[PG_HINGE] = groups(c->n_hinge); nb[PG_TET] = groups(c->n_tet); nb[PG_CONTACT] = groups(nvf);
  nb[PG_STVK] = c->n_stvk > 0 ? groups(c->n_cface) : 0; nb[PG_HANDLE] = groups(c->n_handle);
  PgLayout L;
  if (pg_layout(n_cloth, n_el, nb, need, kr, L, err)) return tsl_fail("%s", err.c_str());
  const PgTiePlace tp = pg_tie_place(L.total, !tie_keys.empty() && c->n_tie > 0 ? nblk(c->n_tie, PG_TIE_THREADS) : 0);
  if (tp.total > (size_t)INT32_MAX) return tsl_fail("tsl_param_grad_keys: too many partials");
  for (int j : tie_keys) { PgTable& tab = L.chunks[j / PG_KEYS_PER_LAUNCH]; tab.off[j % PG_KEYS_PER_LAUNCH] = (int)tp.off; tab.cnt[j % PG_KEYS_PER_LAUNCH] = tp.cnt; }
  if (c->pg_part.n < std::max<size_t>(tp.total, 1)) TSL_TRY(c->pg_part.alloc(std::max<size_t>(tp.total, 1)));
  if (c->pg_out.n < (size_t)n_keys + 2) TSL_TRY(c->pg_out.alloc((size_t)n_keys + 2));
  const double* p = p_dev ? p_dev : c->pdir.p;
  const int* fz = c->frozen.p;
  double* part = c->pg_part.p;
  auto on = [&](PgClass q) { return need[q] && nb[q]; };
  if (on(PG_FACE)) {
    if (c->n_stvk > 0) hipLaunchKernelGGL(k_pg_face<true>, dim3(nb[PG_FACE]), dim3(PG_THREADS), 0, s, cloth_args(c), n_cloth, pos, p, fz, part + L.off[PG_FACE], stvk_args(c));
    else hipLaunchKernelGGL(k_pg_face<false>, dim3(nb[PG_FACE]), dim3(PG_THREADS), 0, s, cloth_args(c), n_cloth, pos, p, fz, part + L.off[PG_FACE], stvk_args(c));
  }
  if (on(PG_HANDLE))
    handle_dispatch(c, [&](auto NC) { hipLaunchKernelGGL(k_pg_handle<NC>, dim3(nb[PG_HANDLE]), dim3(PG_THREADS), 0, s, handle_args(c), pos, p, fz, part + L.off[PG_HANDLE]); });
  if (tp.cnt > 0) hipLaunchKernelGGL(k_pg_tie, dim3(tp.cnt), dim3(PG_TIE_THREADS), 0, s, tie_args(c), pos, p, fz, (double*)nullptr, part + tp.off);
  if (on(PG_STVK)) hipLaunchKernelGGL(k_pg_stvk, dim3(nb[PG_STVK]), dim3(PG_THREADS), 0, s, cloth_args(c), n_cloth, pos, p, fz, part + L.off[PG_STVK], stvk_args(c));
  if (on(PG_HINGE)) hipLaunchKernelGGL(k_pg_hinge, dim3(nb[PG_HINGE]), dim3(PG_THREADS), 0, s, cloth_args(c), n_cloth, pos, ref, p, fz, part + L.off[PG_HINGE]);
  if (on(PG_TET)) hipLaunchKernelGGL(k_pg_tet, dim3(nb[PG_TET]), dim3(PG_THREADS), 0, s, tet_args(c), n_el, pos, p, fz, part + L.off[PG_TET]);
  if (on(PG_CONTACT))
    hipLaunchKernelGGL(k_pg_contact, dim3(nb[PG_CONTACT]), dim3(PG_THREADS), 0, s, nvf, contact_args(c), (const int*)c->c_kind.p, c->mu_cloth_elastic, c->mu_cloth_cloth, pos, p, fz,
                       part + L.off[PG_CONTACT]);
  // the (offset, count) tables as kernel arguments, one launch per chunk of keys; the first launch also counts the kinds of the edge-edge slots -- only
  // when a friction key asks (k_contact with such slots failed above)
  const int n_ee = need[PG_CONTACT] ? c->nc_ee : 0;
  for (size_t k = 0; k < L.chunks.size(); k++) {
    const size_t j0 = k * PG_KEYS_PER_LAUNCH;
    hipLaunchKernelGGL(k_pg_final, dim3(1), dim3(PG_THREADS), 0, s, L.chunks[k], (const double*)part, k == 0 ? n_ee : 0,
                       n_ee > 0 ? (const int*)c->c_kind.p + nvf : (const int*)nullptr, c->pg_out.p + j0, k == 0 ? c->pg_out.p + n_keys : (double*)nullptr);
  }
  HIP_OK(hipGetLastError());
  std::vector<double> h((size_t)n_keys + 2);
  HIP_OK(hipMemcpyAsync(h.data(), c->pg_out.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (int j = 0; j < n_keys; j++) {
    if (kr[j].cls != PG_CONTACT || kr[j].row == PG_ROW_K_CONTACT) continue;
    const double n_kind = h[n_keys + kr[j].row - 1];   // (the count of the slots of kind 1 / 2)
    if (n_kind > 0)
      return tsl_fail("tsl_param_grad_keys: %s: %d edge-edge constraints (contact_ee = 1) use it; their friction derivative is not implemented", keys[j], (int)n_kind);
  }
  for (int j = 0; j < n_keys; j++) out_host[j] = h[j];
  return 0;
}
