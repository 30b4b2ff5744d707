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
// The kernels are k_shape.hpp's with PlaneShape below: one lane per VERTEX, the planes in ascending j, the plane table by value in the kernel
// arguments.  Launched only while colliders exist and k_collider != 0.
#pragma once
#include "collider_host.hpp"
#include "k_contact.hpp"
#include "k_shape.hpp"

// what every kernel needs of the pair (vertex, collider j)
struct ColPair {
  d3 n, t1, t2, w;   // w = T u
  double d, d0, mu, pen, lam, u0, u1, r, f1;
};
TSL_DEV ColPair col_pair(const ColliderPlanes& P, int j, const d3& x, const d3& xp) {
  ColPair c;
  const double* q = P.row[j];
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

struct PlaneShape {
  using Table = ColliderPlanes;
  static constexpr int stride = 3, n_force = 3, n_grad = 2;
  // The upper triangle of H is formed and mirrored (Sym3).  `exact` is not read: both parts of H are positive semi-definite
  static TSL_DEV void assemble(const Table& P, int j, const d3& x, const d3& xp, int, d3& g, Sym3& H) {
    const ColPair c = col_pair(P, j, x, xp);
    if (c.d < P.eps) {
      g = g + c.n * (P.k * (c.d - P.eps));
      H.xx += P.k * (c.n.x * c.n.x); H.xy += P.k * (c.n.x * c.n.y); H.xz += P.k * (c.n.x * c.n.z);
      H.yy += P.k * (c.n.y * c.n.y); H.yz += P.k * (c.n.y * c.n.z); H.zz += P.k * (c.n.z * c.n.z);
    }
    if (c.lam > 0.0) {
      g = g + c.w * (c.lam * c.f1);
      double ha, hb, hd;
      col_core(c, P.eh, ha, hb, hd);
      const d3 a = c.t1 * ha + c.t2 * hb, b = c.t1 * hb + c.t2 * hd;   // rows of core T^T
      H.xx += c.lam * (c.t1.x * a.x + c.t2.x * b.x); H.xy += c.lam * (c.t1.x * a.y + c.t2.x * b.y); H.xz += c.lam * (c.t1.x * a.z + c.t2.x * b.z);
      H.yy += c.lam * (c.t1.y * a.y + c.t2.y * b.y); H.yz += c.lam * (c.t1.y * a.z + c.t2.y * b.z); H.zz += c.lam * (c.t1.z * a.z + c.t2.z * b.z);
    }
  }
  static TSL_DEV void energy(const Table& P, int j, const d3& x, const d3& xp, double& e) {
    const ColPair c = col_pair(P, j, x, xp);
    if (c.d < P.eps) e += 0.5 * P.k * (c.d - P.eps) * (c.d - P.eps);
    if (c.lam > 0.0) e += c.lam * fr_f0(c.r, P.eh);
  }
  // H_f p_v + [d0 < eps] mu k (p_v . f1 T u) n  = -(dg / dx_prev)^T p_v, H_f the friction part of H
  static TSL_DEV void backprop(const Table& P, int j, const d3& x, const d3& xp, const d3& pv, d3& acc) {
    const ColPair c = col_pair(P, j, x, xp);
    if (!(c.lam > 0.0)) return;   // (lam > 0 implies d0 < eps and mu > 0)
    double ha, hb, hd;
    col_core(c, P.eh, ha, hb, hd);
    const double a = dot(c.t1, pv), b = dot(c.t2, pv);
    acc = acc + (c.t1 * (ha * a + hb * b) + c.t2 * (hb * a + hd * b)) * c.lam;
    acc = acc + c.n * ((c.mu * P.k) * (c.f1 * dot(c.w, pv)));
  }
  // tsl_collider_force: -g_v of collider j
  static TSL_DEV void force(const Table& P, int j, const d3& x, const d3& xp, double (&s)[3]) {
    const ColPair c = col_pair(P, j, x, xp);
    d3 g(0.0, 0.0, 0.0);
    if (c.d < P.eps) g = g + c.n * (P.k * (c.d - P.eps));
    if (c.lam > 0.0) g = g + c.w * (c.lam * c.f1);
    s[0] = -g.x; s[1] = -g.y; s[2] = -g.z;
  }
  // tsl_collider_grad: slot 0: -p_v . (-[d < eps] k n + [d0 < eps] mu k f1 T u), this reverse step's share of d(loss)/d(o_j);  slot 1:
  // -p_v . (k max(0, eps - d0) f1 T u), the share of d(loss)/d(mu_j)
  static TSL_DEV void grad(const Table& P, int j, const d3& x, const d3& xp, const d3& pv, double (&s)[2]) {
    const ColPair c = col_pair(P, j, x, xp);
    const double pn = dot(c.n, pv), pw = c.f1 * dot(c.w, pv);
    double so = 0.0;
    if (c.d < P.eps) so += P.k * pn;
    if (c.d0 < P.eps) so -= (c.mu * P.k) * pw;
    s[0] = so;
    s[1] = -((P.k * c.pen) * pw);
  }
};
