// Kernels of the reverse step (Grad.transfer_grad, analytic_grad_single.py:217-257): clamp, ref-angle backprop, tmp_z_frozen, inertia backprop.
#pragma once
#include "k_cloth.hpp"
#include "tsl_device.hpp"

// Grad.clamp_grad (analytic_grad_single.py:176-185)
__global__ void k_clamp(size_t n, double* __restrict__ v, double lim) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) v[i] = fmin(fmax(v[i], -lim), lim);
}

// Cloth.ref_angle_backprop_a2ax (model_fold_offset.py:1179-1206), one lane per hinge.
// ag_s / ag_prev: angleref_grad[s], angleref_grad[s-1]; pg_s: pos_grad[s]; ref = ref_angle_{s-1}; pos = x_s
__global__ void __launch_bounds__(256) k_adj_a2ax(ClothArgs A, const double* __restrict__ pos, const double* __restrict__ ref, const double* __restrict__ ag_s, double* __restrict__ ag_prev) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= A.n_hinge) return;
  const int f1 = A.hg_info[8 * h], l = A.hg_info[8 * h + 1], f2 = A.hg_info[8 * h + 2], p4 = A.hg_info[8 * h + 3], p21 = A.hg_info[8 * h + 4];
  const ClothDev c = A.cloth[A.cid[f1]];
  int v1[3], v2[3]; d3 P1[3], P2[3];
  load_face(pos, A.f2v, f1, v1, P1);
  load_face(pos, A.f2v, f2, v2, P2);
  const FaceGeom g1 = face_geom(P1), g2 = face_geom(P2);
  d3 g[4];
  hinge_grad(g1, g2, l, p4, p21, g);
  const double theta = dihedral(g1.n, g2.n, pick3(P1, (l + 1) % 2) - pick3(P1, l));
  const double a = ag_s[3 * f1 + l];
  ag_prev[3 * f1 + l] += a;
  const double sgn = (fabs(theta - ref[3 * f1 + l]) > c.k_angle) ? a : a * 0.1;
#pragma unroll
  for (int j = 0; j < 4; j++) st3(A.gstage, A.gs_hinge + 4 * h + j, sgn * g[j]);   // staged, summed per vertex by k_vertex_gather
}

// Cloth.ref_angle_backprop_x2a (model_fold_offset.py:1154-1168): angleref_grad[s-1] += -z . (d_ref * grad theta)
__global__ void __launch_bounds__(256) k_adj_x2a(ClothArgs A, const double* __restrict__ pos, const double* __restrict__ z, double* __restrict__ ag_prev) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= A.n_hinge) return;
  const int f1 = A.hg_info[8 * h], l = A.hg_info[8 * h + 1], f2 = A.hg_info[8 * h + 2], p4 = A.hg_info[8 * h + 3], p21 = A.hg_info[8 * h + 4];
  const ClothDev c = A.cloth[A.cid[f1]];
  int v1[3], v2[3]; d3 P1[3], P2[3];
  load_face(pos, A.f2v, f1, v1, P1);
  load_face(pos, A.f2v, f2, v2, P2);
  const FaceGeom g1 = face_geom(P1), g2 = face_geom(P2);
  d3 g[4];
  hinge_grad(g1, g2, l, p4, p21, g);
  const double d_ref = -2.0 * c.Kb * c.dx * c.dx * (1.0 / 3.0);
  const double s = dot(ld3(z, pick3(v1, l)), g[0]) + dot(ld3(z, pick3(v1, (l + 1) % 3)), g[1]) + dot(ld3(z, pick3(v1, (l + 2) % 3)), g[2]) + dot(ld3(z, pick3(v2, p4)), g[3]);
  ag_prev[3 * f1 + l] += -s * d_ref;
}


// The same sums without atomics: one thread per (permuted) row c with a frozen dof walks ITS blocks (c, p); the block that carries the
// contribution is the transposed one, (p, c), found through a static table (trans[slot of (c, p)] = address of block (p, c); the
// pattern is symmetric, the values are not: factor-2 quirk of the area term); fixed order, plain store of the row's three sums
__global__ void k_zfrozen_gather(int NV, const int* __restrict__ slice_off, const int* __restrict__ slice_len, const int* __restrict__ colidx, const int* __restrict__ trans,
                                 const unsigned char* __restrict__ fz, const double* __restrict__ vals, const double* __restrict__ zp, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= NV) return;
  const unsigned cm = fz[c];
  double acc[3] = {0.0, 0.0, 0.0};
  if (cm) {
    const int slice = c >> 6, lane = c & 63, off = slice_off[slice], len = slice_len[slice];
    for (int k = 0; k < len; k++) {
      const int sl = off + 64 * k + lane;
      const int p = colidx[sl];
      const int tb = trans[sl];
      if (tb < 0) continue;   // padding of the slice
      const unsigned rm = fz[p];
      if (rm == 7u) continue;
      const d3 zi = ld3(zp, p);
      const double zr[3] = {zi.x, zi.y, zi.z};
      for (int cc = 0; cc < 3; cc++) {
        if (!((cm >> cc) & 1u)) continue;
        double s = 0;
        for (int r = 0; r < 3; r++) if (!((rm >> r) & 1u)) s += vals[(size_t)tb + 64 * (3 * r + cc)] * zr[r];
        acc[cc] -= s;
      }
    }
  }
  out[3 * (size_t)c] = acc[0]; out[3 * (size_t)c + 1] = acc[1]; out[3 * (size_t)c + 2] = acc[2];
}
// contact part of tmp_z_frozen per vertex (original order) through the row lists of the step's constraints, fixed order
__global__ void __launch_bounds__(256) k_contact_zfrozen_gather(int NV, const int* __restrict__ rowpos, const int* __restrict__ cr_ptr, const int* __restrict__ cr_ent,
                                                                const int* __restrict__ idx, const int* __restrict__ frozen, const double* __restrict__ Hfull,
                                                                const double* __restrict__ z, double* __restrict__ out) {
  const int v = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;   // one wave per vertex, lanes over the row's entries
  if (v >= NV) return;
  const int fz[3] = {frozen[3 * v], frozen[3 * v + 1], frozen[3 * v + 2]};
  if (!(fz[0] | fz[1] | fz[2])) return;
  const int p = rowpos[v];
  const int r0 = cr_ptr[p], r1 = cr_ptr[p + 1];
  if (r1 <= r0) return;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int e = r0 + lane; e < r1; e += 64) {
    const int q = cr_ent[e], ci = q >> 2, a = q & 3;
    const double* H = Hfull + 144 * (size_t)ci;
    for (int cc = 0; cc < 3; cc++) {
      if (!fz[cc]) continue;
      double s = 0;
      for (int k = 0; k < 4; k++) {
        const int u = idx[4 * ci + k];
        for (int j = 0; j < 3; j++) if (!frozen[3 * u + j]) s += H[(3 * k + j) * 12 + 3 * a + cc] * z[3 * (size_t)u + j];
      }
      acc[cc] -= s;
    }
  }
  for (int cc = 0; cc < 3; cc++) { const double t = wave_sum(acc[cc]); if (lane == 0 && fz[cc]) out[3 * (size_t)v + cc] += t; }
}

// x_hat_grad = z m / dt^2 ; pos_grad[s-1] += (1+d) x_hat_grad, pos_grad[s-2] -= d x_hat_grad on free dofs
// (Grad.get_grad / get_prev_grad / get_prev_prev_grad, analytic_grad_single.py:81-106)
__global__ void k_adj_prev(int NV, const double* __restrict__ z, const double* __restrict__ mass, const int* __restrict__ frozen, double dt, double d,
                           double* __restrict__ pg_prev, double* __restrict__ pg_prev2) {
  const size_t n = 3 * (size_t)NV;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (frozen[i]) continue;
    const double xh = z[i] * mass[i / 3] / (dt * dt);
    if (pg_prev) pg_prev[i] += xh * (1.0 + d);
    if (pg_prev2) pg_prev2[i] -= xh * d;
  }
}
