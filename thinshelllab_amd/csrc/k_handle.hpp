// Soft handles (tsl_set_handles, tsl_set_handles_on_faces): handle i has NC corners (v_a, b_a), pulls the point p_i = sum_a b_a x_{v_a}
// to a world-space target t_i with stiffness k_handle w_i,
//   E_h = 1/2 k_handle sum_i w_i |p_i - t_i|^2,  gradient row v_a: k_handle w_i b_a (p_i - t_i),  block (v_a, v_b): k_handle w_i b_a b_b I_3.
// NC = 3: a barycentric point of the face (v_0, v_1, v_2).  NC = 1: the vertex v_0 with b_0 = 1; the coordinate table is not read.  Every kernel is a
// template on NC and the host picks the instance (handle_dispatch, handle_api.hpp).  No counterpart in the reference (its only hold on a vertex is
// set_frozen).
// Any number of handles of a face list may share a face or a vertex, so a row or a block has many contributions: the gradient runs one lane per
// touched VERTEX and the matrix one lane per touched BLOCK over the gather lists of handle_host.hpp, each adding its entries in list order and
// writing once.  The energy, the read-outs and the reductions are one lane per handle.  No atomics: the same bits run to run.  Launched only while
// handles exist and k_handle != 0; without them an assembly, an energy and a reverse step are the launches they were.
// The block is an outer product times I_3 with k, w >= 0: positive semi-definite as it stands, so spd 0 / 1 / 2 and "spd_literal" add the same
// numbers.  Frozen dofs follow the rule of every other term: the kernels add to the unmasked gradient and matrix, k_mask_vec / k_mask_matrix behind
// them take the frozen entries out again (and put m / dt^2 on the frozen diagonal).
#pragma once
#include "tsl_device.hpp"

struct HandleArgs {
  int n;
  const int* cv;      // n x NC  corner vertices of handle i (original numbering)
  const double* cb;   // n x NC  corner coordinates; not read when NC == 1
  const double* w;    // n       weight
  const double* t;    // n x 3   target
  double k;           // k_handle
};
// the gather lists (handle_host.hpp): touched vertices with entries NC i + a, touched blocks with entries NC NC i + NC a + b
struct HandleLists_dev {
  int n_vert, n_blk;
  const int *vl_v, *vl_ptr, *vl_ent;
  const int *bl_addr, *bl_ptr, *bl_ent;
};

// The join of a 256-lane workgroup, N sums at once: the lanes of a wave by wave_sum, then the four waves in order through LDS; lane 0 stores out[0 .. N)
template <int N>
TSL_DEV void wg_join(const double (&s)[N], double* __restrict__ out) {
  __shared__ double sw[4][N];
#pragma unroll
  for (int q = 0; q < N; q++) {
    const double r = wave_sum(s[q]);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6][q] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = ((sw[0][q] + sw[1][q]) + sw[2][q]) + sw[3][q];
  }
}

// p_i = (b_0 x_{v_0} + b_1 x_{v_1}) + b_2 x_{v_2};  NC = 1: x_{v_0}
template <int NC>
TSL_DEV d3 handle_point(const HandleArgs& A, const double* __restrict__ pos, int i) {
  if constexpr (NC == 1) {
    return ld3(pos, A.cv[i]);
  } else {
    const int* __restrict__ v = A.cv + 3 * (size_t)i;
    const double* __restrict__ b = A.cb + 3 * (size_t)i;
    return (ld3(pos, v[0]) * b[0] + ld3(pos, v[1]) * b[1]) + ld3(pos, v[2]) * b[2];
  }
}
// row i of tsl_handle_grad: component c = k w_i sum_a b_a p_{v_a, c} over the corners whose dof (v_a, c) is free, exactly 0 where none is
template <int NC>
TSL_DEV d3 handle_backprop_row(const HandleArgs& A, const double* __restrict__ p, const int* __restrict__ frozen, int i) {
  if constexpr (NC == 1) {
    const int v = A.cv[i];
    const double kw = A.k * A.w[i];
    const d3 pv = ld3(p, v);
    return d3(frozen[3 * v] ? 0.0 : kw * pv.x, frozen[3 * v + 1] ? 0.0 : kw * pv.y, frozen[3 * v + 2] ? 0.0 : kw * pv.z);
  } else {
    const int* __restrict__ v = A.cv + 3 * (size_t)i;
    const double* __restrict__ b = A.cb + 3 * (size_t)i;
    d3 s(0.0, 0.0, 0.0);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const d3 pv = ld3(p, v[a]);
      const int* __restrict__ fz = frozen + 3 * (size_t)v[a];
      s = s + d3(fz[0] ? 0.0 : b[a] * pv.x, fz[1] ? 0.0 : b[a] * pv.y, fz[2] ? 0.0 : b[a] * pv.z);
    }
    return s * (A.k * A.w[i]);
  }
}

// F[v] += sum over the entries (i, a) of v of k w_i b_a (p_i - t_i), in list order, one addition to the row: one lane per touched vertex.  The
// residual is recomputed per entry (nine position loads; no pre-pass launch, no buffer between two launches).  Behind k_vert_grad, which stores the
// row, in front of the gathers and k_mask_vec, on the stream of the vertex terms.
// NC = 1 adds its entries to the row one by one instead -- one entry per vertex (handle_validate), one fused multiply-add per axis: the bits a
// vertex list had while it ran one lane per handle.
template <int NC>
__global__ void k_handle_grad(HandleArgs A, HandleLists_dev L, const double* __restrict__ pos, double* __restrict__ F) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_vert) return;
  const int v = L.vl_v[q];
  if constexpr (NC == 1) {
    d3 r = ld3(F, v);
    for (int e = L.vl_ptr[q], e1 = L.vl_ptr[q + 1]; e < e1; e++) {
      const int i = L.vl_ent[e];
      r = r + (ld3(pos, v) - ld3(A.t, i)) * (A.k * A.w[i]);
    }
    st3(F, v, r);
  } else {
    d3 s(0.0, 0.0, 0.0);
    for (int e = L.vl_ptr[q], e1 = L.vl_ptr[q + 1]; e < e1; e++) {
      const int ia = L.vl_ent[e], i = ia / 3;
      s = s + (handle_point<3>(A, pos, i) - ld3(A.t, i)) * ((A.k * A.w[i]) * A.cb[ia]);
    }
    st3(F, v, ld3(F, v) + s);
  }
}

// diagonal of block (v_a, v_b) += sum over the block's entries (i, a, b) of (k w_i) (b_a b_b), in list order: one lane per touched block.  Blocks
// (v_a, v_b) and (v_b, v_a) hold the same handles in the same order and b_a b_b commutes: the handle part is symmetric bit for bit.  Behind
// k_vert_hess (one writer at a time per block, all on one stream), in front of the gathers and k_mask_matrix -- block Jacobi, the body inverses, the
// multigrid operators and the factorisation read the masked copy.  NC = 1: k w_i added to the entries one by one, as in k_handle_grad.
template <int NC>
__global__ void k_handle_hess(HandleArgs A, HandleLists_dev L, double* __restrict__ vals) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_blk) return;
  const size_t base = (size_t)L.bl_addr[q];
  if constexpr (NC == 1) {
    for (int e = L.bl_ptr[q], e1 = L.bl_ptr[q + 1]; e < e1; e++) {
      const double kw = A.k * A.w[L.bl_ent[e]];
      vals[base + 64 * 0] += kw;
      vals[base + 64 * 4] += kw;
      vals[base + 64 * 8] += kw;
    }
  } else {
    double s = 0.0;
    for (int e = L.bl_ptr[q], e1 = L.bl_ptr[q + 1]; e < e1; e++) {
      const int iab = L.bl_ent[e], i = iab / 9, ab = iab - 9 * i;
      s += (A.k * A.w[i]) * (A.cb[3 * (size_t)i + ab / 3] * A.cb[3 * (size_t)i + ab % 3]);
    }
    vals[base + 64 * 0] += s;
    vals[base + 64 * 4] += s;
    vals[base + 64 * 8] += s;
  }
}

// one partial per workgroup, joined like energy_body's (wg_join); k_energy_final adds the partials (behind the contact ones) in its fixed order
template <int NC>
__global__ void __launch_bounds__(256) k_handle_energy(HandleArgs A, const double* __restrict__ pos, double* __restrict__ e_part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  if (i < A.n) {
    const d3 d = handle_point<NC>(A, pos, i) - ld3(A.t, i);
    e[0] = 0.5 * (A.k * A.w[i]) * dot(d, d);
  }
  wg_join<1>(e, e_part + blockIdx.x);
}

// tsl_handle_points: out[i] = p_i
template <int NC>
__global__ void k_handle_points(HandleArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, handle_point<NC>(A, pos, i));
}

// tsl_handle_force: out[i] = k w_i (t_i - p_i), the force the handle applies to the cloth; frozen dofs are not masked (a read-out)
template <int NC>
__global__ void k_handle_force(HandleArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, (ld3(A.t, i) - handle_point<NC>(A, pos, i)) * (A.k * A.w[i]));
}

// tsl_handle_grad: out[i] = -p . dF/dt_i
template <int NC>
__global__ void k_handle_backprop(HandleArgs A, const double* __restrict__ p, const int* __restrict__ frozen, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, handle_backprop_row<NC>(A, p, frozen, i));
}
