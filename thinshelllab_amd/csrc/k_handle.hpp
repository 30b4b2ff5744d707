// Soft handles (tsl_set_handles): handle i is a spring of stiffness k_handle w_i from vertex v_i to a world-space target t_i,
//   E_h = 1/2 k_handle sum_i w_i |x_{v_i} - t_i|^2,  gradient row v_i: k_handle w_i (x - t),  diagonal block of v_i: k_handle w_i I_3.
// No counterpart in the reference (its only hold on a vertex is set_frozen).  At most one handle per vertex (tsl_set_handles checks), so every
// kernel below is one lane per handle with plain loads and stores: no atomics, the same bits run to run.  They are launched only while handles
// exist and k_handle != 0; without them an assembly, an energy and a reverse step are the launches they were.
// The block is k w I_3 with k, w >= 0: positive semi-definite as it stands, so spd 0 / 1 / 2 and "spd_literal" add the same three numbers.
// Frozen dofs follow the rule of every other term: the kernels add to the unmasked gradient and matrix, k_mask_vec / k_mask_matrix behind them
// take the frozen entries out again (and put m / dt^2 on the frozen diagonal).
#pragma once
#include "tsl_device.hpp"

struct HandleArgs {
  int n;
  const int* v;       // n    vertex of handle i (original numbering)
  const double* w;    // n    weight
  const double* t;    // n x 3 target
  double k;           // k_handle
};

// F[v_i] += k w_i (x - t_i): behind k_vert_grad (which stores the row), in front of the gathers and k_mask_vec, on the stream of the vertex terms
__global__ void k_handle_grad(HandleArgs A, const double* __restrict__ pos, double* __restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int v = A.v[i];
  const double kw = A.k * A.w[i];
  st3(F, v, ld3(F, v) + (ld3(pos, v) - ld3(A.t, i)) * kw);
}

// diagonal block of v_i += k w_i I_3: behind k_vert_hess (one writer at a time per diagonal block, all on one stream), in front of the gathers and
// k_mask_matrix -- block Jacobi, the body inverses, the multigrid operators and the factorisation read the masked copy
__global__ void k_handle_hess(HandleArgs A, const int* __restrict__ diag_blk, double* __restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const double kw = A.k * A.w[i];
  const int base = diag_blk[A.v[i]];
  vals[(size_t)base + 64 * 0] += kw;
  vals[(size_t)base + 64 * 4] += kw;
  vals[(size_t)base + 64 * 8] += kw;
}

// one partial per workgroup, joined like energy_body's: the lanes of a wave by wave_sum, then the four waves in order; k_energy_final adds the
// partials (behind the contact ones) in its fixed order
__global__ void __launch_bounds__(256) k_handle_energy(HandleArgs A, const double* __restrict__ pos, double* __restrict__ e_part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double e = 0;
  if (i < A.n) {
    const d3 d = ld3(pos, A.v[i]) - ld3(A.t, i);
    e = 0.5 * (A.k * A.w[i]) * dot(d, d);
  }
  e = wave_sum(e);
  __shared__ double sw[4];
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) e_part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// tsl_handle_force: out[i] = k w_i (t_i - x_{v_i}), the force the handle applies to the cloth; frozen dofs are not masked (a read-out)
__global__ void k_handle_force(HandleArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, (ld3(A.t, i) - ld3(pos, A.v[i])) * (A.k * A.w[i]));
}

// tsl_handle_grad: out[i] = -p . dF/dt_i = k w_i p_{v_i} on the free dofs of v_i, exactly 0 on the frozen ones
__global__ void k_handle_backprop(HandleArgs A, const double* __restrict__ p, const int* __restrict__ frozen, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int v = A.v[i];
  const double kw = A.k * A.w[i];
  const d3 pv = ld3(p, v);
  st3(out, i, d3(frozen[3 * v] ? 0.0 : kw * pv.x, frozen[3 * v + 1] ? 0.0 : kw * pv.y, frozen[3 * v + 2] ? 0.0 : kw * pv.z));
}
