// Read-only views of the iterative hierarchy and entry points that run one of its parts alone (tests/ only; declared in tsl_hip.h).
// Included by tsl_hip.hip behind the solvers: every function here calls the static functions of that file and launches nothing of its own
// besides the gather / scatter between the caller's vertex order and the solver's.
#pragma once

// the set-up a solve runs before its first preconditioner application, in pcg_restarts' order
static int pc_prepare(tsl_ctx* c) {
  TSL_TRY(block_jacobi_ensure(c));
  if (body_active(c) && !c->bd_valid) TSL_TRY(body_build_inverse(c));
  if (mg_active(c) && !c->mg_ops_valid) TSL_TRY(mg_setup_operators(c));
  return 0;
}

// how the cycle solves level l of mc: 0 not the last level, 1 dense inverse, 2 one-workgroup k_st_coarse, 3 one launch per sweep (mg_stencil_cycle's rule)
static int mg_level_kind(tsl_ctx* c, MgCloth* mc, size_t l) {
  MgLevel* L = mc->lv[l];
  if (l + 1 < mg_levels(c, mc)) return 0;
  if (L->n <= 64 || mg_level_dense(c, L)) return (mg_level_dense(c, L) && L->Cinv.n > 0) ? 1 : 2;
  return 3;
}

extern "C" int tsl_mg_info(tsl_ctx* c, int32_t* out, int32_t cap) {
  std::vector<int32_t> v;
  if (mg_active(c) && !c->mg_ops_valid) {   // (the dense inverse of a last level is allocated by the set-up: the kind of that level depends on it)
    Scope scope(c);
    TSL_TRY(pc_prepare(c));
    HIP_OK(hipStreamSynchronize(c->stream));
  }
  const bool mg = mg_active(c);
  v.push_back(mg ? (int32_t)c->mg.size() : 0);
  const bool bd = body_active(c);
  v.push_back(bd ? c->bd_args.nb : 0);
  if (mg)
    for (MgCloth* mc : c->mg) {
      const size_t nl = mg_levels(c, mc);
      v.push_back(mc->v_offset); v.push_back(mc->N0); v.push_back(mc->M0); v.push_back((int32_t)nl);
      for (size_t l = 0; l < nl; l++) { v.push_back(mc->lv[l]->N); v.push_back(mc->lv[l]->M); v.push_back(mg_level_kind(c, mc, l)); }
    }
  if (bd)
    for (int b = 0; b < c->bd_args.nb; b++) v.push_back(c->bd_args.n3[b]);
  if ((int32_t)v.size() > cap) return tsl_fail("tsl_mg_info: %d values, room for %d", (int)v.size(), (int)cap);
  std::copy(v.begin(), v.end(), out);
  return (int)v.size();
}

template <class T>
static int mg_copy_out(tsl_ctx* c, const T* dev, size_t n, void* host, long cap, const char* what) {
  if (!dev || n == 0) return tsl_fail("tsl_mg_export: no %s on this level", what);
  if ((long)n > cap) return tsl_fail("tsl_mg_export: %s has %ld entries, room for %ld", what, (long)n, cap);
  HIP_OK(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return (int)n;
}

extern "C" int tsl_mg_export(tsl_ctx* c, int32_t hierarchy, int32_t level, int32_t what, void* host, int64_t cap) {
  Scope scope(c);
  TSL_TRY(pc_prepare(c));
  if (what == TSL_MG_BINV || what == TSL_MG_BAD_BODY) {
    const BodyDenseArgs& A = c->bd_args;
    if (!(body_active(c) && c->bd_valid) || hierarchy < 0 || hierarchy >= A.nb) return tsl_fail("tsl_mg_export: no dense body %d", (int)hierarchy);
    if (what == TSL_MG_BAD_BODY) return mg_copy_out(c, c->bd_bad.p + hierarchy, 1, host, cap, "bd_bad");
    return mg_copy_out(c, c->bd_Binv.p + A.w_off[hierarchy], (size_t)A.n3[hierarchy] * ((A.n3[hierarchy] + 3) & ~3), host, cap, "Binv");
  }
  if (!mg_active(c)) return tsl_fail("tsl_mg_export: the multigrid preconditioner is not active");
  if (level < 0) {
    if (what == TSL_MG_OMEGA) return mg_copy_out(c, c->mg_omega0.p, 2, host, cap, "omega0");
    if (what == TSL_MG_ROWPOS) return mg_copy_out(c, c->rowpos.p, (size_t)c->NV, host, cap, "rowpos");
    if (what != TSL_MG_DINV) return tsl_fail("tsl_mg_export: level -1 has Dinv, omega and rowpos only");
    const size_t n = 9 * (size_t)c->NV;
    if ((long)n > cap) return tsl_fail("tsl_mg_export: Dinv has %ld entries, room for %ld", (long)n, (long)cap);
    std::vector<double> h(n);
    HIP_OK(hipMemcpyAsync(h.data(), c->Dinv.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    double* o = (double*)host;
    for (int v = 0; v < c->NV; v++) std::copy(h.begin() + 9 * (size_t)c->h_rowpos[v], h.begin() + 9 * (size_t)c->h_rowpos[v] + 9, o + 9 * (size_t)v);
    return (int)n;
  }
  if (hierarchy < 0 || hierarchy >= (int)c->mg.size()) return tsl_fail("tsl_mg_export: no hierarchy %d", (int)hierarchy);
  MgCloth* mc = c->mg[hierarchy];
  if (level >= (int)mg_levels(c, mc)) return tsl_fail("tsl_mg_export: hierarchy %d has %d levels", (int)hierarchy, (int)mg_levels(c, mc));
  MgLevel* L = mc->lv[level];
  const bool last = level + 1 == (int)mg_levels(c, mc);
  const int kind = mg_level_kind(c, mc, level);
  switch (what) {
    case TSL_MG_A: return mg_copy_out(c, L->A.p, (size_t)225 * L->n, host, cap, "A");
    case TSL_MG_DINV: return mg_copy_out(c, L->Dinv.p, (size_t)9 * L->n, host, cap, "Dinv");
    case TSL_MG_OMEGA: return mg_copy_out(c, kind == 1 ? (const double*)nullptr : L->omega.p, 2, host, cap, "omega");
    case TSL_MG_A32: return mg_copy_out(c, last ? (const float*)nullptr : L->A32.p, (size_t)225 * L->n, host, cap, "A32");
    case TSL_MG_S32: return mg_copy_out(c, last ? (const float*)nullptr : L->S32.p, last ? 0 : (size_t)441 * mc->lv[level + 1]->n, host, cap, "S32");
    case TSL_MG_CINV: return mg_copy_out(c, kind == 1 ? L->Cinv.p : (const float*)nullptr, (size_t)9 * L->n * L->n, host, cap, "Cinv");
    case TSL_MG_BAD: return mg_copy_out(c, kind == 1 ? L->cbad.p : (const int*)nullptr, 1, host, cap, "cbad");
  }
  return tsl_fail("tsl_mg_export: unknown array %d", (int)what);
}

extern "C" int tsl_mg_apply(tsl_ctx* c, const double* r_dev, double* z_dev) {
  Scope scope(c);
  hipStream_t s = c->stream;
  const int NV = c->NV, gb = nblk(NV, 256);
  TSL_TRY(pc_prepare(c));
  hipLaunchKernelGGL(k_gather_perm, dim3(gb), dim3(256), 0, s, NV, c->perm.p, r_dev, c->v_r.p);
  if (mg_active(c)) mg_vcycle(c, c->v_r.p, c->v_z.p, c->part_rz.p);
  else {
    hipLaunchKernelGGL(k_precond, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, c->v_r.p, c->v_z.p);
    if (body_active(c) && c->bd_valid) body_apply(c, 0, c->v_r.p, nullptr, c->v_z.p, nullptr, nullptr);
  }
  hipLaunchKernelGGL(k_scatter_perm, dim3(gb), dim3(256), 0, s, NV, c->perm.p, c->v_z.p, z_dev);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

extern "C" int tsl_solve_with(tsl_ctx* c, int32_t method, int32_t cap, const double* rhs_dev, double* x_dev, tsl_solve_stats* st) {
  if (method < 0 || method > 3) return tsl_fail("tsl_solve_with: method %d (0 PCG, 1 MINRES, 2 GMRES, 3 BiCGStab)", (int)method);
  Scope scope(c);
  hipStream_t s = c->stream;
  const int gb = nblk(c->NV, 256);
  tsl_solve_stats local;
  if (!st) st = &local;
  if (cap <= 0) cap = c->cg_maxit;
  hipLaunchKernelGGL(k_gather_perm, dim3(gb), dim3(256), 0, s, c->NV, c->perm.p, rhs_dev, c->v_b.p);
  solve_stats_reset(c, st);
  {
    Suspend hierarchy_runs(c->ds_suspended);   // as wherever solve_direct runs the hierarchy
    if (method == 0) {
      PcgOutcome pcg;
      TSL_TRY(pcg_restarts(c, st, cap, &pcg));
      st->flag = pcg.need_fallback ? 3 : 0;
    } else {
      TSL_TRY(block_jacobi_ensure(c));   // (pcg_restarts does this for the solvers behind it)
      if (method == 1) TSL_TRY(minres(c, st, cap));
      else if (method == 2) TSL_TRY(gmres(c, st, cap));
      else TSL_TRY(bicgstab(c, st, cap));
    }
  }
  st->method = method;
  hipLaunchKernelGGL(k_scatter_perm, dim3(gb), dim3(256), 0, s, c->NV, c->perm.p, c->v_x.p, x_dev);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}
