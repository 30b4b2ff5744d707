// Kernels of a scene as a whole: the total energy (BaseScene.compute_energy) as per-workgroup partials joined in a fixed order, and the gathers of the
// deterministic gradient -- staged element gradients and contact rows summed per vertex.
#pragma once
#include "k_cloth.hpp"
#include "k_fem.hpp"
#include "tsl_device.hpp"

template <bool STVK>   // STVK: some cloth has membrane = 1 (cface_energy_sel)
TSL_DEV void energy_body(VertArgs VA, ClothArgs CA, TetArgs TA, const double* __restrict__ pos, const double* __restrict__ prev,
                         const double* __restrict__ vel, const double* __restrict__ ref_angle, double* __restrict__ e_part, StvkArgs S) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  double e = 0;
  if (t < VA.NV) e += vert_energy(VA, t, pos, prev, vel);
  if (t < CA.n_cface) {
    int v[3]; d3 P[3];
    load_face(pos, CA.f2v, t, v, P);
    const double li[3] = {CA.li[3 * t], CA.li[3 * t + 1], CA.li[3 * t + 2]};
    if constexpr (STVK) e += cface_energy_sel(CA.cloth[CA.cid[t]], S.stvk + 4 * CA.cid[t], S.dminv + 4 * t, P, CA.V[t], li);
    else e += cface_energy(CA.cloth[CA.cid[t]], P, CA.V[t], li);
  }
  if (t < CA.n_hinge) e += hinge_energy(CA, t, pos, ref_angle);
  if (t < TA.n_tet) e += tet_energy(TA, t, pos);
  e = wave_sum(e);
  // the four waves of the workgroup in order, one partial per workgroup; k_energy_final adds the partials in order
  __shared__ double sw[4];
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) e_part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}
__global__ void k_energy(VertArgs VA, ClothArgs CA, TetArgs TA, const double* __restrict__ pos, const double* __restrict__ prev,
                         const double* __restrict__ vel, const double* __restrict__ ref_angle, double* __restrict__ e_part) {
  energy_body<false>(VA, CA, TA, pos, prev, vel, ref_angle, e_part, StvkArgs{nullptr, nullptr});
}
__global__ void k_energy_stvk(VertArgs VA, ClothArgs CA, TetArgs TA, const double* __restrict__ pos, const double* __restrict__ prev,
                              const double* __restrict__ vel, const double* __restrict__ ref_angle, double* __restrict__ e_part, StvkArgs S) {
  energy_body<true>(VA, CA, TA, pos, prev, vel, ref_angle, e_part, S);
}
// sum of n partial energies in a fixed order (one workgroup: strided per-thread sums, then a fixed tree)
__global__ void __launch_bounds__(256) k_energy_final(int n, const double* __restrict__ part, double* __restrict__ e_out) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += part[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) *e_out = sh[0];
}

// Deterministic gradient: F[v] (holding the vertex term) += the staged gradients of the faces, hinges and tets at v (static lists, ascending
// slot) + the rows of the contact constraints at v (the step's row lists, ascending constraint and slot), in this order
__global__ void k_vertex_gather(int NV, const int* __restrict__ vg_ptr, const int* __restrict__ vg_idx, const double* __restrict__ stage, int lo, int hi, double* __restrict__ F) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= NV) return;
  d3 a = ld3(F, v);
  for (int e = vg_ptr[v]; e < vg_ptr[v + 1]; e++) { const int i = vg_idx[e]; if (i >= lo && i < hi) a = a + ld3(stage, i); }   // staging slots in [lo, hi) only
  st3(F, v, a);
}
// ... and the contact part: one WAVE per vertex, lanes over the entries of its row (l, l + 64, ...: a table vertex under a folded cloth has
// hundreds), joined by the fixed tree of wave_sum; cg: per-constraint 12-vectors
__global__ void __launch_bounds__(256) k_contact_row_gather(int NV, const int* __restrict__ rowpos, const int* __restrict__ cr_ptr, const int* __restrict__ cr_ent,
                                                            const double* __restrict__ cg, double* __restrict__ F) {
  const int v = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (v >= NV) return;
  const int p = rowpos[v];
  const int r0 = cr_ptr[p], r1 = cr_ptr[p + 1];
  if (r1 <= r0) return;
  double a0 = 0, a1 = 0, a2 = 0;
  for (int e = r0 + lane; e < r1; e += 64) {
    const int q = cr_ent[e];
    const double* g = cg + 12 * (size_t)(q >> 2) + 3 * (q & 3);
    a0 += g[0]; a1 += g[1]; a2 += g[2];
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
  if (lane == 0) st3(F, v, ld3(F, v) + d3(a0, a1, a2));
}
