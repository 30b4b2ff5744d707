// The collider layer that the kinds share: everything of a collider kernel that is not geometry.  A kind -- planes (k_collider.hpp),
// balls (k_sphere.hpp), rods (k_capsule.hpp), rounded boxes (k_box.hpp), sampled distance fields (k_sdf.hpp) -- is a struct Shape of static device functions and constants:
//   Table              its ShapeTable (shape_host.hpp) or a type derived from it (SdfTable), by value in the kernel arguments
//   stride             slots of one shape in the partial buffer of the read-outs (>= n_force, n_grad)
//   n_force, n_grad    values per shape of the two read-outs
//   assemble(T, j, x, xp, exact, g, H)   g += the pair's gradient, H += its 3 x 3 block
//   energy(T, j, x, xp, e)               e += the pair's energy
//   backprop(T, j, x, xp, pv, acc)       acc += -(dg / dx_prev)^T pv
//   force(T, j, x, xp, s)                s[0 .. n_force) = the pair's share of the force read-out (s comes in as zeros)
//   grad(T, j, x, xp, pv, s)             s[0 .. n_grad)  = the pair's share of the gradient read-out (likewise)
// for the pair (vertex at x, start-of-step position xp; shape j of the table T).  The kernels here own the frame: one lane per VERTEX, a vertex
// with mask 0 leaves at once, the shapes in ascending j, one write per vertex, joins per workgroup (wg_join).  No atomics, every sum in a fixed
// order: the same bits run to run.  Frozen dofs follow the rule of every other term: the assembly adds to the unmasked gradient and matrix,
// k_mask_vec / k_mask_matrix behind it take the frozen entries out again; the adjoint solution counts on its free dofs only (free_p).
#pragma once
#include "k_handle.hpp"
#include "shape_host.hpp"
#include "tsl_device.hpp"

struct ShapeArgs {
  int NV;
  const unsigned char* mask;   // NV: bit j set: shape j acts on the vertex
};

// The upper triangle of a symmetric 3 x 3 block; stamp mirrors it into the vertex's diagonal block (diag_blk, as k_vert_hess and the vertex
// handles do), so that the block is symmetric bit for bit
struct Sym3 {
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  TSL_DEV void stamp(double* __restrict__ vals, size_t base) const {
    vals[base + 64 * 0] += xx; vals[base + 64 * 1] += xy; vals[base + 64 * 2] += xz;
    vals[base + 64 * 3] += xy; vals[base + 64 * 4] += yy; vals[base + 64 * 5] += yz;
    vals[base + 64 * 6] += xz; vals[base + 64 * 7] += yz; vals[base + 64 * 8] += zz;
  }
};

// p with its frozen dofs zeroed
TSL_DEV d3 free_p(const int* __restrict__ frozen, const double* __restrict__ p, int v) {
  const int* __restrict__ fz = frozen + 3 * (size_t)v;
  const d3 pr = ld3(p, v);
  return d3(fz[0] ? 0.0 : pr.x, fz[1] ? 0.0 : pr.y, fz[2] ? 0.0 : pr.z);
}
// row v of pg += acc on its free dofs
TSL_DEV void add_free(const int* __restrict__ frozen, double* __restrict__ pg, int v, const d3& acc) {
  const int* __restrict__ fz = frozen + 3 * (size_t)v;
  const d3 o = ld3(pg, v);
  st3(pg, v, d3(fz[0] ? o.x : o.x + acc.x, fz[1] ? o.y : o.y + acc.y, fz[2] ? o.z : o.z + acc.z));
}

// F[v] += g (where a gradient is asked for), diagonal block of v += H.  exact (uniform): spd == 0, a kind whose H has an indefinite part adds it;
// else that part is left out.  Behind k_vert_grad / k_vert_hess on their stream, in front of the gathers and the masks (in front of ev_fork in the
// three-stream schedule).
template <class Shape>
__global__ void __launch_bounds__(256) k_shape_assemble(typename Shape::Table T, ShapeArgs A, int exact, const double* __restrict__ pos, const double* __restrict__ prev,
                                                        const int* __restrict__ diag_blk, double* __restrict__ F, double* __restrict__ vals) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= A.NV) return;
  const unsigned m = A.mask[v];
  if (!m) return;
  const d3 x = ld3(pos, v), xp = ld3(prev, v);
  d3 g(0.0, 0.0, 0.0);
  Sym3 H;
  for (int j = 0; j < T.n; j++) {
    if (!((m >> j) & 1u)) continue;
    Shape::assemble(T, j, x, xp, exact, g, H);
  }
  if (F) st3(F, v, ld3(F, v) + g);
  H.stamp(vals, (size_t)diag_blk[v]);
}

// one partial per workgroup (wg_join); k_energy_final adds them in its fixed order
template <class Shape>
__global__ void __launch_bounds__(256) k_shape_energy(typename Shape::Table T, ShapeArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                      double* __restrict__ e_part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  if (m) {
    const d3 x = ld3(pos, v), xp = ld3(prev, v);
    for (int j = 0; j < T.n; j++) {
      if (!((m >> j) & 1u)) continue;
      Shape::energy(T, j, x, xp, e[0]);
    }
  }
  wg_join<1>(e, e_part + blockIdx.x);
}

// The reverse step: pos = x_s, prev = x_{s-1}, p the adjoint solution (its frozen dofs do not count), the table as it stood in step s.  Into the
// vertex's own row of pos_grad[s-1], on free dofs:  += sum_j -(dg / dx_prev)^T p_v.  In front of k_adj_prev.
template <class Shape>
__global__ void __launch_bounds__(256) k_shape_backprop(typename Shape::Table T, ShapeArgs A, const int* __restrict__ frozen, const double* __restrict__ pos,
                                                        const double* __restrict__ prev, const double* __restrict__ p, double* __restrict__ pg_prev) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= A.NV) return;
  const unsigned m = A.mask[v];
  if (!m) return;
  const d3 pv = free_p(frozen, p, v);
  const d3 x = ld3(pos, v), xp = ld3(prev, v);
  d3 acc(0.0, 0.0, 0.0);
  for (int j = 0; j < T.n; j++) {
    if (!((m >> j) & 1u)) continue;
    Shape::backprop(T, j, x, xp, pv, acc);
  }
  add_free(frozen, pg_prev, v, acc);
}

// Read-outs.  A workgroup writes SHAPE_MAX * stride partials, stride per shape; the shapes are joined one after the other, so that a lane holds
// the sums of one shape at a time; k_shape_join adds the partials in workgroup order.
// Shape::force: the net force the shape applies to the cloth, -sum_v g_v (the sign of k_handle_force); frozen dofs are not masked
template <class Shape>
__global__ void __launch_bounds__(256) k_shape_force(typename Shape::Table T, ShapeArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                     double* __restrict__ part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  d3 x, xp;
  if (m) { x = ld3(pos, v); xp = ld3(prev, v); }
  for (int j = 0; j < T.n; j++) {   // (uniform)
    double s[Shape::n_force];
#pragma unroll
    for (int q = 0; q < Shape::n_force; q++) s[q] = 0.0;
    if ((m >> j) & 1u) Shape::force(T, j, x, xp, s);
    wg_join<Shape::n_force>(s, part + (size_t)(SHAPE_MAX * Shape::stride) * blockIdx.x + Shape::stride * j);
    __syncthreads();   // (the LDS of wg_join is used again for the next shape)
  }
}
// Shape::grad: this reverse step's share of d(loss)/d(the shape's parameters), each -sum_v (dg/d.)^T p_v.  Free dofs of p only.
template <class Shape>
__global__ void __launch_bounds__(256) k_shape_grad(typename Shape::Table T, ShapeArgs A, const int* __restrict__ frozen, const double* __restrict__ pos,
                                                    const double* __restrict__ prev, const double* __restrict__ p, double* __restrict__ part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  d3 pv, x, xp;
  if (m) { pv = free_p(frozen, p, v); x = ld3(pos, v); xp = ld3(prev, v); }
  for (int j = 0; j < T.n; j++) {   // (uniform)
    double s[Shape::n_grad];
#pragma unroll
    for (int q = 0; q < Shape::n_grad; q++) s[q] = 0.0;
    if ((m >> j) & 1u) Shape::grad(T, j, x, xp, pv, s);
    wg_join<Shape::n_grad>(s, part + (size_t)(SHAPE_MAX * Shape::stride) * blockIdx.x + Shape::stride * j);
    __syncthreads();   // (the LDS of wg_join is used again for the next shape)
  }
}
// out[per j + i] = part[0][stride j + i] + part[1][stride j + i] + ..., in workgroup order, for j < n, i < per: one lane per slot (SHAPE_MAX * stride
// lanes).  A slot's sum is the same whatever shares its join: wg_join reduces each slot on its own (wave_sum, then the four waves in order), and
// this kernel adds the workgroups of a slot in index order, so neither the number of slots of a wg_join nor the stride enters a sum.
__global__ void k_shape_join(int n_wg, int n, int per, int stride, const double* __restrict__ part, double* __restrict__ out) {
  const int q = threadIdx.x, j = q / stride, i = q - stride * j;
  if (j >= n || i >= per) return;
  double t = 0.0;
  for (int w = 0; w < n_wg; w++) t += part[(size_t)(SHAPE_MAX * stride) * w + q];
  out[per * j + i] = t;
}
