// The operator the Krylov solvers iterate on, taken apart (tests/ only; declared in tsl_hip.h): its tables and values as the next solve reads them, one
// product by each kernel that forms it, and the first iterations of a PCG run with every vector, partial sum and scalar of the state behind them.
// Included by tsl_hip.hip behind mg_test_api.hpp: every function here calls the static functions and kernels of that file and launches nothing of its own
// besides the gather / scatter between the caller's vertex order and the solver's.
#pragma once

template <class T>
static int op_copy_out(tsl_ctx* c, const T* dev, size_t n, void* host, int64_t cap, const char* what) {
  if ((int64_t)n > cap) return tsl_fail("tsl_op_export: %s has %ld entries, room for %ld", what, (long)n, (long)cap);
  if (n == 0) return 0;
  if (!dev) return tsl_fail("tsl_op_export: %s is not allocated", what);
  HIP_OK(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return (int)n;
}

extern "C" int tsl_op_export(tsl_ctx* c, int32_t what, void* host, int64_t cap) {
  Scope scope(c);
  const size_t NV = (size_t)c->NV, nc4 = c->nc > 0 ? 4 * (size_t)c->nc : 0;
  switch (what) {
    case TSL_OP_SLICE_OFF: return op_copy_out(c, c->slice_off.p, c->slice_off.n, host, cap, "slice_off");
    case TSL_OP_SLICE_LEN: return op_copy_out(c, c->slice_len.p, c->slice_len.n, host, cap, "slice_len");
    case TSL_OP_COLIDX: return op_copy_out(c, c->colidx.p, c->colidx.n, host, cap, "colidx");
    case TSL_OP_PERM: return op_copy_out(c, c->perm.p, NV, host, cap, "perm");
    case TSL_OP_ROWPOS: return op_copy_out(c, c->rowpos.p, NV, host, cap, "rowpos");
    case TSL_OP_DIAG_PERM: return op_copy_out(c, c->diag_perm.p, NV, host, cap, "diag_perm");
    case TSL_OP_VALS: return op_copy_out(c, c->vals.p, c->vals.n, host, cap, "vals");
    case TSL_OP_VALS_FULL: return op_copy_out(c, c->vals_full.p, c->vals_full.n, host, cap, "vals_full");
    case TSL_OP_FZMASK: return op_copy_out(c, c->fzmask.p, NV, host, cap, "fzmask");
    case TSL_OP_MDT2: return op_copy_out(c, c->mdt2.p, NV, host, cap, "mdt2");
    case TSL_OP_DINV:    // through the solver's own "is it stale" test: a flag that should have been cleared shows as the inverse of the previous values
      TSL_TRY(block_jacobi_ensure(c));
      return op_copy_out(c, c->Dinv.p, 9 * NV, host, cap, "Dinv");
    case TSL_OP_CDIAG:
      TSL_TRY(block_jacobi_ensure(c));
      return op_copy_out(c, c->c_diag.p, c->nc > 0 ? 9 * NV : 0, host, cap, "c_diag");
    case TSL_OP_CR_PTR: return op_copy_out(c, c->cr_ptr.p, c->nc > 0 ? NV + 1 : 0, host, cap, "cr_ptr");
    case TSL_OP_CR_ENT: return op_copy_out(c, c->cr_ent.p, nc4, host, cap, "cr_ent");
    case TSL_OP_CR_ROWS: return op_copy_out(c, (const int*)c->cr_rows.p, 4 * nc4, host, cap, "cr_rows");
  }
  return tsl_fail("tsl_op_export: unknown array %d", (int)what);
}

extern "C" int tsl_op_apply(tsl_ctx* c, int32_t kernel, const double* x_dev, double* y_dev, double* dot_host, double* part_host, int32_t cap) {
  if (kernel < 0 || kernel > 9) return tsl_fail("tsl_op_apply: kernel %d (0 k_spmv + k_contact_matvec, 1..7 the variants of tsl_bench_spmv, 8 launch_spmv, 9 the same with partials)", (int)kernel);
  Scope scope(c);
  hipStream_t s = c->stream;
  const int NV = c->NV, gb = nblk(NV, 256), ns = c->n_slices;
  double* x = c->v_p.p;     // (the vectors tsl_bench_spmv works on)
  double* y = c->v_Ap.p;
  double* part = kernel == 9 ? c->part_pAp.p : c->v_t4.p;
  int n_part = 0;
  hipLaunchKernelGGL(k_gather_perm, dim3(gb), dim3(256), 0, s, NV, c->perm.p, x_dev, x);
  HIP_OK(hipMemsetAsync(c->scal.p, 0, sizeof(SolverScalars), s));
  if (kernel <= 7) {
    n_part = spmv_variant_launch(c, kernel, x, y, part);
    if (kernel == 0 && c->nc > 0)
      hipLaunchKernelGGL(k_contact_matvec, dim3(nblk(c->nc, 64)), dim3(CONTACT_MV_THREADS), 0, s, c->nc, c->c_idx.p, c->rowpos.p, c->c_H.p, x, y, SC(c), 0, 0);
  } else if (kernel == 8) launch_spmv(c, c->vals.p, x, y, -1, 0);
  else {   // launch_minres_iteration's product: the kernel of launch_spmv with the partials of x . H x and the stop flag of the scalar record (zero here)
    hipLaunchKernelGGL((k_spmv_mw<4, 1, TSL_NT>), dim3(ns), dim3(256), 0, s, NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, &MSC(c)->flag,
                       contact_rows(c, c->c_H.p));
    n_part = ns;
  }
  hipLaunchKernelGGL(k_scatter_perm, dim3(gb), dim3(256), 0, s, NV, c->perm.p, y, y_dev);
  HIP_OK(hipGetLastError());
  if (n_part > cap) return tsl_fail("tsl_op_apply: %d partials, room for %d", n_part, (int)cap);
  if (n_part > 0) HIP_OK(hipMemcpyAsync(part_host, part, (size_t)n_part * sizeof(double), hipMemcpyDeviceToHost, s));
  TSL_TRY(read_scal(c));
  if (dot_host) *dot_host = HSC(c)->pAp[0];
  return n_part;
}

// out_vec: 6 vectors of 3 * tot_NV in the solver's (permuted) order: x, r, z, p of the last iteration, p of the one before, Ap.
// out_part: 3 arrays of cap_part doubles: the partials of p.Ap, r.z and r.r; n_part[3] their counts.
// out_scal[11]: rzh[0], rzh[1], thresh2, bb, rr_last, rz_last, pAp_last, flag, iters, n_part1, n_part2.  Returns the chunk of the graph.
extern "C" int tsl_pcg_trace(tsl_ctx* c, const double* rhs_dev, int32_t n_iter, int32_t use_graph, double* out_vec, double* out_part, int32_t cap_part, int32_t* n_part,
                             double* out_scal) {
  if (n_iter < 1) return tsl_fail("tsl_pcg_trace: n_iter %d", (int)n_iter);
  Scope scope(c);
  hipStream_t s = c->stream;
  const int NV = c->NV, gb = nblk(NV, 256);
  const size_t n3 = 3 * (size_t)NV;
  hipLaunchKernelGGL(k_gather_perm, dim3(gb), dim3(256), 0, s, NV, c->perm.p, rhs_dev, c->v_b.p);
  double bb = 0;
  TSL_TRY(pcg_begin(c, &bb));
  if (!(bb > 0)) return tsl_fail("tsl_pcg_trace: the right-hand side is zero");
  // what pcg_restarts runs at outer == 0, with a threshold nothing meets
  TSL_TRY(pcg_start_residual(c, bb, -1.0, false));
  TSL_TRY(pcg_start_precond(c));
  launch_pcg_iteration(c, 0, 1, nullptr);
  const int chunk = pcg_chunk(c);
  if (use_graph) {
    if ((n_iter - 1) % chunk) return tsl_fail("tsl_pcg_trace: %d iterations behind the first are no multiple of the chunk of %d", (int)n_iter - 1, chunk);
    TSL_TRY(pcg_chunk_graph(c, chunk));
    for (int k = 0; k < (n_iter - 1) / chunk; k++) HIP_OK(hipGraphLaunch(c->pcg_graph, s));
  } else
    for (int i = 0; i < n_iter - 1; i++) launch_pcg_iteration(c, (i & 1) ^ 1, 0, nullptr);
  HIP_OK(hipGetLastError());
  const int last = (n_iter - 1) & 1;   // parity of the last iteration: its p is in v_t0 if odd
  const double* vec[6] = {c->v_x.p, c->v_r.p, c->v_z.p, last ? c->v_t0.p : c->v_p.p, last ? c->v_p.p : c->v_t0.p, c->v_Ap.p};
  for (int k = 0; k < 6; k++) HIP_OK(hipMemcpyAsync(out_vec + k * n3, vec[k], n3 * sizeof(double), hipMemcpyDeviceToHost, s));
  const int np[3] = {c->n_slices, pcg_n_rz(c), gb};
  const double* pp[3] = {c->part_pAp.p, c->part_rz.p, c->part_rr.p};
  for (int k = 0; k < 3; k++) {
    if (np[k] > cap_part) return tsl_fail("tsl_pcg_trace: %d partials, room for %d", np[k], (int)cap_part);
    HIP_OK(hipMemcpyAsync(out_part + (size_t)k * cap_part, pp[k], (size_t)np[k] * sizeof(double), hipMemcpyDeviceToHost, s));
    n_part[k] = np[k];
  }
  TSL_TRY(read_scal(c));
  const PcgScal* h = HPSC(c);
  const double sc[11] = {h->rzh[0], h->rzh[1], h->thresh2, h->bb, h->rr_last, h->rz_last, h->pAp_last, (double)h->flag, (double)h->iters, (double)h->n_part1, (double)h->n_part2};
  std::copy(sc, sc + 11, out_scal);
  return chunk;
}
