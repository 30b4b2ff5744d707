// Ties (tsl_set_ties): tie i binds vertex v_i to the point with barycentric coordinates b_i on face (t0, t1, t2),
//   r_i = x_v - sum_a b_a x_{t_a},   E_tie = 1/2 k_tie sum_i w_i |r_i|^2.
// In the vertex order (t0, t1, t2, v) of a constraint slot with c = (-b0, -b1, -b2, 1): gradient on corner a: k_tie w_i c_a r_i, 12 x 12 block:
// k_tie w_i (c c^T) (x) I_3 -- constant and positive semi-definite as it stands, so no projection, every spd mode and "spd_literal" add the same
// numbers, and the adjoint's un-projected operator is the same block.  A tie couples vertices that share no element, so it is not in the static
// block pattern: ties are a third class of constraint slots behind the vertex-triangle and the edge-edge ones (k_contact.hpp), [nc - nc_tie, nc),
// and everything that works by slot -- mask, row lists, row gather, matrix-free product, diagonal, the cliques of the factorisation plan -- takes
// them as it takes the others.  The kernels here read the context's own copy of the list (idx n x 4, b n x 3, w n), not the slots.
// No atomics, every sum in a fixed order: the same bits run to run.  Launched only while ties exist and k_tie != 0.
#pragma once
#include "tsl_device.hpp"

struct TieArgs {
  int n;
  const int* idx;     // n x 4  (t0, t1, t2, v), original numbering
  const double* b;    // n x 3  barycentric coordinates of the point on the face
  const double* w;    // n      weight
  double k;           // k_tie
};

// c_a of corner a of tie i: (-b0, -b1, -b2, 1)
TSL_DEV double tie_c(const TieArgs& A, int i, int a) { return a < 3 ? -A.b[3 * (size_t)i + a] : 1.0; }
// r_i = x_v - ((b0 x_t0 + b1 x_t1) + b2 x_t2)
TSL_DEV d3 tie_residual(const TieArgs& A, const double* __restrict__ pos, int i) {
  const int* __restrict__ v = A.idx + 4 * (size_t)i;
  const double* __restrict__ b = A.b + 3 * (size_t)i;
  return ld3(pos, v[3]) - ((ld3(pos, v[0]) * b[0] + ld3(pos, v[1]) * b[1]) + ld3(pos, v[2]) * b[2]);
}

// The tie slots appended behind the detected ones (the slot arrays point at the first tie slot): idx and w from the list, no friction (c_k = c_mu = 0,
// c_kind = 0), dx0, T, n zero.  One lane per (tie, j), j < 6: lane j of a tie stores entry j of every array that has one, so the lanes of a wave
// store to consecutive addresses of each array.
__global__ void k_tie_slots(TieArgs A, int* __restrict__ c_idx, double* __restrict__ c_w, double* __restrict__ c_n, double* __restrict__ c_dx0, double* __restrict__ c_k,
                            double* __restrict__ c_mu, double* __restrict__ c_T, int* __restrict__ c_kind) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * (long)A.n) return;
  const int i = (int)(t / 6), j = (int)(t % 6);
  c_T[t] = 0.0;
  if (j < 4) c_idx[4 * (size_t)i + j] = A.idx[4 * (size_t)i + j];
  if (j < 3) { c_w[3 * (size_t)i + j] = A.b[3 * (size_t)i + j]; c_n[3 * (size_t)i + j] = 0.0; c_dx0[3 * (size_t)i + j] = 0.0; }
  if (j == 0) { c_k[i] = 0.0; c_mu[i] = 0.0; c_kind[i] = 0; }
}

// The 144 entries of the unmasked block of every tie slot, one lane per ENTRY (a wave stores 64 consecutive doubles): entry (r, q) =
// (k w) (c_{r/3} c_{q/3}) where r % 3 == q % 3, else 0 -- the product of the two coordinates commutes, so the block is symmetric bit for bit.
// With cg: the first twelve lanes of a tie also store its gradient, entry 3 a + x = ((k w) c_a) r_x (summed per vertex by k_contact_row_gather).
// Hfull, cg point at the first tie slot.  Behind the two contact assemblies on their stream, in front of k_contact_mask.
__global__ void __launch_bounds__(256) k_tie_assemble(TieArgs A, const double* __restrict__ pos, double* __restrict__ Hfull, double* __restrict__ cg) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 144 * (long)A.n) return;
  const int i = (int)(t / 144), e = (int)(t % 144), r = e / 12, q = e % 12;
  const double kw = A.k * A.w[i];
  Hfull[t] = (r % 3 == q % 3) ? kw * (tie_c(A, i, r / 3) * tie_c(A, i, q / 3)) : 0.0;
  if (cg && e < 12) {
    const d3 res = tie_residual(A, pos, i);
    cg[12 * (size_t)i + e] = (kw * tie_c(A, i, e / 3)) * res[e % 3];
  }
}

// One partial per WAVE: wave j of workgroup g writes e_part[4 g + j] (waves past the last tie write nothing: nblk(n, 64) partials in all), summed
// in order by k_energy_final behind the edge-edge partials
__global__ void __launch_bounds__(256) k_tie_energy(TieArgs A, const double* __restrict__ pos, double* __restrict__ e_part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double e = 0.0;
  if (i < A.n) {
    const d3 r = tie_residual(A, pos, i);
    e = 0.5 * (A.k * A.w[i]) * dot(r, r);
  }
  e = wave_sum(e);
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if ((threadIdx.x & 63) == 0 && wave * 64 < A.n) e_part[wave] = e;
}

// tsl_tie_residuals: out[i] = r_i
__global__ void k_tie_residual(TieArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, tie_residual(A, pos, i));
}

// tsl_tie_force: out[i] = -k w_i r_i, the force the tie applies to its vertex; frozen dofs are not masked (a read-out)
__global__ void k_tie_force(TieArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, tie_residual(A, pos, i) * (-(A.k * A.w[i])));
}

// The parameter pass of the ties: g_i = -sum_a sum_{c free} p_{a, c} c_a r_{i, c}, the gradient rows of k_tie_assemble with k w = 1 dotted with p at
// the free dofs, one lane per tie.  out (tsl_tie_grad; may be null): out[i] = k g_i, the contribution of one reverse step to d(loss)/d(w_i).
// part (the "k_tie" key; may be null): one partial sum_i w_i g_i per workgroup, joined by the fixed tree of block_sum; k_pg_final adds them.
#define PG_TIE_THREADS 256
__global__ void __launch_bounds__(PG_TIE_THREADS) k_pg_tie(TieArgs A, const double* __restrict__ pos, const double* __restrict__ p, const int* __restrict__ frozen,
                                                           double* __restrict__ out, double* __restrict__ part) {
  __shared__ double sm[PG_TIE_THREADS / 64];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double g = 0.0;
  if (i < A.n) {
    const d3 r = tie_residual(A, pos, i);
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int v = A.idx[4 * (size_t)i + a];
      const double ca = tie_c(A, i, a);
      if (!frozen[3 * v]) s += p[3 * (size_t)v] * (ca * r.x);
      if (!frozen[3 * v + 1]) s += p[3 * (size_t)v + 1] * (ca * r.y);
      if (!frozen[3 * v + 2]) s += p[3 * (size_t)v + 2] * (ca * r.z);
    }
    g = -s;
    if (out) out[i] = A.k * g;
  }
  if (part) {   // (uniform over the workgroup: block_sum synchronises)
    const double s = block_sum(i < A.n ? A.w[i] * g : 0.0, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}
