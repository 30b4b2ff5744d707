// Half-space colliders (tsl_set_colliders): collider j is the half-space n_j . x < o_j with a fixed unit normal, an offset that may be
// set before every step, and a friction coefficient mu_j.  For vertex v (position x, start-of-step position x_prev) and collider j, with
// k = "k_collider", eps = eps_contact, eh = eps_v dt:
//   d = n . x - o,  d0 = n . x_prev - o,  lam = mu k max(0, eps - d0)  (the lagged normal force),  u = T^T (x - x_prev),  r = |u|,
//   E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r)
//   g = [d < eps] k (d - eps) n + lam f1(r) T u
//   H = [d < eps] k n n^T + lam T (f1 I + [r > 1e-9] (f2 / r) u u^T) T^T
// with fr_f0 / fr_f1 / fr_f2 of k_contact.hpp and T = (t1, t2) built on the host from n as k_contact_pair builds c_T (collider_host.hpp).  Both parts
// of H are positive semi-definite (f1 >= 0, f1 + f2 r >= 0): no projection, every spd mode and "spd_literal" add the same numbers and the reverse
// step's un-projected operator holds the same block.  H is 3 x 3 on the vertex's own diagonal block: no constraint slot, no row list, no change
// of a factorisation plan.  Nothing is stored per step: everything is a function of (x, x_prev, o), and the normal term is evaluated for every
// masked vertex at every evaluation, so a vertex that reaches a plane in the middle of a step is caught.
// One lane per VERTEX, the planes in ascending j, the plane table by value in the kernel arguments.  A vertex with mask 0 leaves at once.  No
// atomics, every sum in a fixed order: the same bits run to run.  Launched only while colliders exist and k_collider != 0.
// Frozen dofs follow the rule of every other term: the assembly adds to the unmasked gradient and matrix, k_mask_vec / k_mask_matrix behind it take
// the frozen entries out again.
#pragma once
#include "collider_host.hpp"
#include "k_contact.hpp"
#include "k_handle.hpp"
#include "tsl_device.hpp"

struct ColliderArgs {
  int NV;
  const unsigned char* mask;   // NV: bit j set: collider j acts on the vertex
};

// what every kernel needs of the pair (vertex, collider j)
struct ColPair {
  d3 n, t1, t2, w;   // w = T u
  double d, d0, mu, pen, lam, u0, u1, r, f1;
};
TSL_DEV ColPair col_pair(const ColliderPlanes& P, int j, const d3& x, const d3& xp) {
  ColPair c;
  const double* q = P.pl[j];
  c.n = d3(q[0], q[1], q[2]); c.mu = q[4]; c.t1 = d3(q[5], q[6], q[7]); c.t2 = d3(q[8], q[9], q[10]);
  c.d = dot(c.n, x) - q[3];
  c.d0 = dot(c.n, xp) - q[3];
  c.pen = fmax(0.0, P.eps - c.d0);
  c.lam = (c.mu * P.k) * c.pen;
  const d3 dx = x - xp;
  c.u0 = dot(c.t1, dx); c.u1 = dot(c.t2, dx);
  c.r = sqrt(c.u0 * c.u0 + c.u1 * c.u1);
  c.f1 = fr_f1(c.r, P.eh);
  c.w = c.t1 * c.u0 + c.t2 * c.u1;
  return c;
}
// the 2 x 2 core f1 I + [r > 1e-9] (f2 / r) u u^T of the friction block: (ha, hb; hb, hd)
TSL_DEV void col_core(const ColPair& c, double eh, double& ha, double& hb, double& hd) {
  ha = c.f1; hb = 0.0; hd = c.f1;
  if (c.r > 1e-9) {
    const double f2 = fr_f2(c.r, eh);
    ha += f2 * c.u0 * c.u0 / c.r; hb += f2 * c.u0 * c.u1 / c.r; hd += f2 * c.u1 * c.u1 / c.r;
  }
}

// F[v] += g (where a gradient is asked for), diagonal block of v += H through diag_blk, as k_vert_hess and the vertex handles do.  The upper
// triangle of H is formed and mirrored: the block is symmetric bit for bit.  Behind k_vert_grad / k_vert_hess on their stream, in front of the
// gathers and the masks (in front of ev_fork in the three-stream schedule).
__global__ void __launch_bounds__(256) k_collider_assemble(ColliderPlanes P, ColliderArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                           const int* __restrict__ diag_blk, double* __restrict__ F, double* __restrict__ vals) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= A.NV) return;
  const unsigned m = A.mask[v];
  if (!m) return;
  const d3 x = ld3(pos, v), xp = ld3(prev, v);
  d3 g(0.0, 0.0, 0.0);
  double hxx = 0.0, hxy = 0.0, hxz = 0.0, hyy = 0.0, hyz = 0.0, hzz = 0.0;
  for (int j = 0; j < P.n; j++) {
    if (!((m >> j) & 1u)) continue;
    const ColPair c = col_pair(P, j, x, xp);
    if (c.d < P.eps) {
      g = g + c.n * (P.k * (c.d - P.eps));
      hxx += P.k * (c.n.x * c.n.x); hxy += P.k * (c.n.x * c.n.y); hxz += P.k * (c.n.x * c.n.z);
      hyy += P.k * (c.n.y * c.n.y); hyz += P.k * (c.n.y * c.n.z); hzz += P.k * (c.n.z * c.n.z);
    }
    if (c.lam > 0.0) {
      g = g + c.w * (c.lam * c.f1);
      double ha, hb, hd;
      col_core(c, P.eh, ha, hb, hd);
      const d3 a = c.t1 * ha + c.t2 * hb, b = c.t1 * hb + c.t2 * hd;   // rows of core T^T
      hxx += c.lam * (c.t1.x * a.x + c.t2.x * b.x); hxy += c.lam * (c.t1.x * a.y + c.t2.x * b.y); hxz += c.lam * (c.t1.x * a.z + c.t2.x * b.z);
      hyy += c.lam * (c.t1.y * a.y + c.t2.y * b.y); hyz += c.lam * (c.t1.y * a.z + c.t2.y * b.z); hzz += c.lam * (c.t1.z * a.z + c.t2.z * b.z);
    }
  }
  if (F) st3(F, v, ld3(F, v) + g);
  const size_t base = (size_t)diag_blk[v];
  vals[base + 64 * 0] += hxx; vals[base + 64 * 1] += hxy; vals[base + 64 * 2] += hxz;
  vals[base + 64 * 3] += hxy; vals[base + 64 * 4] += hyy; vals[base + 64 * 5] += hyz;
  vals[base + 64 * 6] += hxz; vals[base + 64 * 7] += hyz; vals[base + 64 * 8] += hzz;
}

// one partial per workgroup (wg_join), behind the tie partials; k_energy_final adds them in its fixed order
__global__ void __launch_bounds__(256) k_collider_energy(ColliderPlanes P, ColliderArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                         double* __restrict__ e_part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  if (m) {
    const d3 x = ld3(pos, v), xp = ld3(prev, v);
    for (int j = 0; j < P.n; j++) {
      if (!((m >> j) & 1u)) continue;
      const ColPair c = col_pair(P, j, x, xp);
      if (c.d < P.eps) e[0] += 0.5 * P.k * (c.d - P.eps) * (c.d - P.eps);
      if (c.lam > 0.0) e[0] += c.lam * fr_f0(c.r, P.eh);
    }
  }
  wg_join<1>(e, e_part + blockIdx.x);
}

// The reverse step: pos = x_s, prev = x_{s-1}, p the adjoint solution (its frozen dofs do not count).  Into the vertex's own row of pos_grad[s-1], on
// free dofs:  += sum_j H_f p_v + [d0 < eps] mu k (p_v . f1 T u) n  = -(dg / dx_prev)^T p_v, H_f the friction part of H.  In front of k_adj_prev.
__global__ void __launch_bounds__(256) k_collider_backprop(ColliderPlanes P, ColliderArgs A, const int* __restrict__ frozen, const double* __restrict__ pos,
                                                           const double* __restrict__ prev, const double* __restrict__ p, double* __restrict__ pg_prev) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= A.NV) return;
  const unsigned m = A.mask[v];
  if (!m) return;
  const int* __restrict__ fz = frozen + 3 * (size_t)v;
  const bool f0 = fz[0] != 0, f1 = fz[1] != 0, f2 = fz[2] != 0;
  const d3 pr = ld3(p, v);
  const d3 pv(f0 ? 0.0 : pr.x, f1 ? 0.0 : pr.y, f2 ? 0.0 : pr.z);
  const d3 x = ld3(pos, v), xp = ld3(prev, v);
  d3 acc(0.0, 0.0, 0.0);
  for (int j = 0; j < P.n; j++) {
    if (!((m >> j) & 1u)) continue;
    const ColPair c = col_pair(P, j, x, xp);
    if (!(c.lam > 0.0)) continue;   // (lam > 0 implies d0 < eps and mu > 0)
    double ha, hb, hd;
    col_core(c, P.eh, ha, hb, hd);
    const double a = dot(c.t1, pv), b = dot(c.t2, pv);
    acc = acc + (c.t1 * (ha * a + hb * b) + c.t2 * (hb * a + hd * b)) * c.lam;
    acc = acc + c.n * ((c.mu * P.k) * (c.f1 * dot(c.w, pv)));
  }
  const d3 o = ld3(pg_prev, v);
  st3(pg_prev, v, d3(f0 ? o.x : o.x + acc.x, f1 ? o.y : o.y + acc.y, f2 ? o.z : o.z + acc.z));
}

// Read-outs.  Both write COLLIDER_SLOTS partials per workgroup (wg_join); k_collider_join adds them in workgroup order.  The loops over the planes
// are unrolled over all TSL_MAX_COLLIDERS so that every sum has a register of its own.
#define COLLIDER_SLOTS (3 * TSL_MAX_COLLIDERS)
// tsl_collider_grad: slot 2 j: -sum_v p_v . (-[d < eps] k n + [d0 < eps] mu k f1 T u), this reverse step's share of d(loss)/d(o_j);  slot 2 j + 1:
// -sum_v p_v . (k max(0, eps - d0) f1 T u), the share of d(loss)/d(mu_j).  Free dofs of p only.
__global__ void __launch_bounds__(256) k_collider_grad(ColliderPlanes P, ColliderArgs A, const int* __restrict__ frozen, const double* __restrict__ pos,
                                                       const double* __restrict__ prev, const double* __restrict__ p, double* __restrict__ part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  double s[COLLIDER_SLOTS];
#pragma unroll
  for (int q = 0; q < COLLIDER_SLOTS; q++) s[q] = 0.0;
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  if (m) {
    const int* __restrict__ fz = frozen + 3 * (size_t)v;
    const d3 pr = ld3(p, v);
    const d3 pv(fz[0] ? 0.0 : pr.x, fz[1] ? 0.0 : pr.y, fz[2] ? 0.0 : pr.z);
    const d3 x = ld3(pos, v), xp = ld3(prev, v);
#pragma unroll
    for (int j = 0; j < TSL_MAX_COLLIDERS; j++) {
      if (j < P.n && ((m >> j) & 1u)) {
        const ColPair c = col_pair(P, j, x, xp);
        const double pn = dot(c.n, pv), pw = c.f1 * dot(c.w, pv);
        double so = 0.0;
        if (c.d < P.eps) so += P.k * pn;
        if (c.d0 < P.eps) so -= (c.mu * P.k) * pw;
        s[2 * j] = so;
        s[2 * j + 1] = -((P.k * c.pen) * pw);
      }
    }
  }
  wg_join<COLLIDER_SLOTS>(s, part + (size_t)COLLIDER_SLOTS * blockIdx.x);
}
// tsl_collider_force: slots 3 j .. 3 j + 2: -sum_v g_v of collider j, the net force the plane applies to the cloth (the sign of k_handle_force); frozen dofs
// are not masked
__global__ void __launch_bounds__(256) k_collider_force(ColliderPlanes P, ColliderArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                        double* __restrict__ part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  double s[COLLIDER_SLOTS];
#pragma unroll
  for (int q = 0; q < COLLIDER_SLOTS; q++) s[q] = 0.0;
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  if (m) {
    const d3 x = ld3(pos, v), xp = ld3(prev, v);
#pragma unroll
    for (int j = 0; j < TSL_MAX_COLLIDERS; j++) {
      if (j < P.n && ((m >> j) & 1u)) {
        const ColPair c = col_pair(P, j, x, xp);
        d3 g(0.0, 0.0, 0.0);
        if (c.d < P.eps) g = g + c.n * (P.k * (c.d - P.eps));
        if (c.lam > 0.0) g = g + c.w * (c.lam * c.f1);
        s[3 * j] = -g.x; s[3 * j + 1] = -g.y; s[3 * j + 2] = -g.z;
      }
    }
  }
  wg_join<COLLIDER_SLOTS>(s, part + (size_t)COLLIDER_SLOTS * blockIdx.x);
}
// out[q] = part[0][q] + part[1][q] + ..., in workgroup order: one lane per slot
__global__ void k_collider_join(int n_wg, const double* __restrict__ part, double* __restrict__ out) {
  const int q = threadIdx.x;
  if (q >= COLLIDER_SLOTS) return;
  double t = 0.0;
  for (int w = 0; w < n_wg; w++) t += part[(size_t)COLLIDER_SLOTS * w + q];
  out[q] = t;
}
