// Soft handles at barycentric points of faces (tsl_set_handles_on_faces): handle i sits on face (v_0, v_1, v_2) with barycentric
// coordinates b_i and pulls the point p_i = sum_a b_a x_{v_a} to a world-space target t_i with stiffness k_handle w_i,
//   E_h = 1/2 k_handle sum_i w_i |p_i - t_i|^2,  gradient row v_a: k_handle w_i b_a (p_i - t_i),  block (v_a, v_b): k_handle w_i b_a b_b I_3.
// Any number of handles may share a face or a vertex, so a row or a block has many contributions: the gradient runs one lane per touched VERTEX and
// the matrix one lane per touched BLOCK over the gather lists of handle_face_host.hpp, each adding its entries in list order and writing once.  The
// energy, the read-outs and the reductions are one lane per handle, joined as their vertex counterparts (k_handle.hpp, k_frame.hpp, k_param.hpp)
// join.  No atomics: the same bits run to run.  Launched only while a face list exists and k_handle != 0, at the places of the vertex-handle kernels.
// The block is an outer product times I_3 with k, w >= 0: positive semi-definite as it stands, every spd mode adds the same numbers.  Frozen dofs
// follow the mask rule: the kernels add to the unmasked gradient and matrix, k_mask_vec / k_mask_matrix behind them take the frozen entries out.
#pragma once
#include "k_frame.hpp"
#include "k_handle.hpp"
#include "k_param.hpp"
#include "tsl_device.hpp"

struct FaceHandleArgs {
  int n;
  const int* fv;      // n x 3  vertices of the face of handle i (original numbering)
  const double* b;    // n x 3  barycentric coordinates
  const double* w;    // n      weight
  const double* t;    // n x 3  target
  double k;           // k_handle
};
// the gather lists (handle_face_host.hpp): touched vertices with entries 3 i + a, touched blocks with entries 9 i + 3 a + b
struct FaceHandleLists_dev {
  int n_vert, n_blk;
  const int *vl_v, *vl_ptr, *vl_ent;
  const int *bl_addr, *bl_ptr, *bl_ent;
};

// p_i = (b_0 x_{v_0} + b_1 x_{v_1}) + b_2 x_{v_2}
TSL_DEV d3 hf_point(const FaceHandleArgs& A, const double* __restrict__ pos, int i) {
  const int* __restrict__ v = A.fv + 3 * (size_t)i;
  const double* __restrict__ b = A.b + 3 * (size_t)i;
  return (ld3(pos, v[0]) * b[0] + ld3(pos, v[1]) * b[1]) + ld3(pos, v[2]) * b[2];
}
// row i of tsl_handle_grad: component c = k w_i sum_a b_a p_{v_a, c} over the corners whose dof (v_a, c) is free
TSL_DEV d3 hf_backprop_row(const FaceHandleArgs& A, const double* __restrict__ p, const int* __restrict__ frozen, int i) {
  const int* __restrict__ v = A.fv + 3 * (size_t)i;
  const double* __restrict__ b = A.b + 3 * (size_t)i;
  d3 s(0.0, 0.0, 0.0);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const d3 pv = ld3(p, v[a]);
    const int* __restrict__ fz = frozen + 3 * (size_t)v[a];
    s = s + d3(fz[0] ? 0.0 : b[a] * pv.x, fz[1] ? 0.0 : b[a] * pv.y, fz[2] ? 0.0 : b[a] * pv.z);
  }
  return s * (A.k * A.w[i]);
}

// F[v] += sum over the entries (i, a) of v of k w_i b_a (p_i - t_i), in list order, one addition to the row: one lane per touched vertex.  The
// residual is recomputed per entry (nine position loads; no pre-pass launch, no buffer between two launches).  Behind k_vert_grad, which stores the
// row, in front of the gathers and k_mask_vec, on the stream of the vertex terms.
__global__ void k_hface_grad(FaceHandleArgs A, FaceHandleLists_dev L, const double* __restrict__ pos, double* __restrict__ F) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_vert) return;
  d3 s(0.0, 0.0, 0.0);
  for (int e = L.vl_ptr[q], e1 = L.vl_ptr[q + 1]; e < e1; e++) {
    const int ia = L.vl_ent[e], i = ia / 3;
    s = s + (hf_point(A, pos, i) - ld3(A.t, i)) * ((A.k * A.w[i]) * A.b[ia]);
  }
  const int v = L.vl_v[q];
  st3(F, v, ld3(F, v) + s);
}

// diagonal of block (v_a, v_b) += sum over the block's entries (i, a, b) of (k w_i) (b_a b_b), in list order: one lane per touched block.  Blocks
// (v_a, v_b) and (v_b, v_a) hold the same handles in the same order and b_a b_b commutes: the handle part is symmetric bit for bit.  Behind
// k_vert_hess (one writer at a time per block, all on one stream), in front of the gathers and k_mask_matrix.
__global__ void k_hface_hess(FaceHandleArgs A, FaceHandleLists_dev L, double* __restrict__ vals) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_blk) return;
  double s = 0.0;
  for (int e = L.bl_ptr[q], e1 = L.bl_ptr[q + 1]; e < e1; e++) {
    const int iab = L.bl_ent[e], i = iab / 9, ab = iab - 9 * i;
    s += (A.k * A.w[i]) * (A.b[3 * (size_t)i + ab / 3] * A.b[3 * (size_t)i + ab % 3]);
  }
  const size_t base = (size_t)L.bl_addr[q];
  vals[base + 64 * 0] += s;
  vals[base + 64 * 4] += s;
  vals[base + 64 * 8] += s;
}

// one partial per workgroup, the join of k_handle_energy: the lanes of a wave by wave_sum, then the four waves in order
__global__ void __launch_bounds__(256) k_hface_energy(FaceHandleArgs A, const double* __restrict__ pos, double* __restrict__ e_part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double e = 0;
  if (i < A.n) {
    const d3 d = hf_point(A, pos, i) - ld3(A.t, i);
    e = 0.5 * (A.k * A.w[i]) * dot(d, d);
  }
  e = wave_sum(e);
  __shared__ double sw[4];
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) e_part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// tsl_handle_points: out[i] = p_i; the vertex list's version reads x_{v_i}
__global__ void k_hface_points(FaceHandleArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, hf_point(A, pos, i));
}
__global__ void k_handle_points(HandleArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, ld3(pos, A.v[i]));
}

// tsl_handle_force: out[i] = k w_i (t_i - p_i); frozen dofs are not masked (a read-out)
__global__ void k_hface_force(FaceHandleArgs A, const double* __restrict__ pos, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, (ld3(A.t, i) - hf_point(A, pos, i)) * (A.k * A.w[i]));
}

// tsl_handle_grad: out[i] = -p . dF/dt_i
__global__ void k_hface_backprop(FaceHandleArgs A, const double* __restrict__ p, const int* __restrict__ frozen, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  st3(out, i, hf_backprop_row(A, p, frozen, i));
}

// {k_handle} of tsl_param_grad_keys on a face list (class 5 of k_param.hpp): -w_i sum_a b_a p_{v_a} . (p_i - t_i) over free dofs; one lane per handle
__global__ void __launch_bounds__(PG_THREADS) k_pg_hface(FaceHandleArgs A, const double* __restrict__ pos, const double* __restrict__ p,
                                                         const int* __restrict__ frozen, double* __restrict__ part) {
  __shared__ double sm[PG_THREADS / 64];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double v[1] = {0.0};
  if (i < A.n) {
    const d3 r = hf_point(A, pos, i) - ld3(A.t, i);
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) s += pg_dot_free(p, frozen, A.fv[3 * (size_t)i + a], r * (A.w[i] * A.b[3 * (size_t)i + a]));
    v[0] = -s;
  }
  pg_block_write<1>(v, i < A.n ? 0 : -1, 1, part, sm);
}

// The two reductions of k_frame_reduce over a face list: f_i the row of k_hface_force (FRAME_WRENCH, vec = positions) or of k_hface_backprop
// (FRAME_GRAD, vec = the adjoint solution); arms, lane order and join as there.
template <int MODE>
__global__ void __launch_bounds__(256) k_hface_frame_reduce(FaceHandleArgs H, FrameArgs A, const double* __restrict__ vec, const int* __restrict__ frozen,
                                                            double* __restrict__ out) {
  const int j = blockIdx.x;
  const int e1 = A.ptr[j + 1];
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double* __restrict__ R = A.R + 9 * (size_t)j;
  const d3 c = MODE == FRAME_WRENCH ? ld3(A.c, j) : d3(0.0, 0.0, 0.0);
  for (int e = A.ptr[j] + (int)threadIdx.x; e < e1; e += 256) {
    const int i = A.idx[e];
    d3 f, a;
    if (MODE == FRAME_WRENCH) {
      const d3 t = ld3(H.t, i);
      f = (t - hf_point(H, vec, i)) * (H.k * H.w[i]);
      a = t - c;
    } else {
      const d3 r = ld3(A.local, i);
      f = hf_backprop_row(H, vec, frozen, i);
      a = d3(R[0] * r.x + R[1] * r.y + R[2] * r.z, R[3] * r.x + R[4] * r.y + R[5] * r.z, R[6] * r.x + R[7] * r.y + R[8] * r.z);
    }
    const d3 m = cross(a, f);
    s[0] += f.x; s[1] += f.y; s[2] += f.z;
    s[3] += m.x; s[4] += m.y; s[5] += m.z;
  }
  __shared__ double sw[4][6];
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const double r = wave_sum(s[q]);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6][q] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 6; q++) out[6 * (size_t)j + q] = ((sw[0][q] + sw[1][q]) + sw[2][q]) + sw[3][q];
  }
}
