// Rounded-box colliders (tsl_set_boxes): box j is a solid box with rounded edges and corners and the cloth outside -- the rod of
// k_capsule.hpp generalised from one slab axis to three.  Centre c and rotation matrix R (columns u_i: the box axes in the world; may be set before
// every step), previous pose cp, R0 (where the box was at the start of the step), half extents h_i >= 0, rounding radius r > 0, friction mu.  For
// vertex v (position x, start-of-step position x_prev) and box j, with k = "k_box", eps = eps_contact, eh = eps_v dt:
//   y  = R^T (x - c),        b  = clamp(y, -h, h),    free_i  = [-h_i < y_i < h_i]
//   q  = R (y - b),  rho = |q|,  n = q / rho,  d = rho - r
//   y0 = R0^T (x_prev - cp), b0 = clamp(y0, -h, h),   free0_i = [-h_i < y0_i < h_i]
//   q0 = R0 (y0 - b0), rho0, n0, d0 = rho0 - r
//   lam = mu k max(0, eps - d0)  (the lagged normal force)
//   dc  = (c + R b0) - (cp + R0 b0)                     the motion of the box's material point under the vertex
//   D   = (x - x_prev) - dc,  P0 = I - n0 n0^T,  w = P0 D,  r_w = |w|,  a1 = f1(r_w),  f2r = [r_w > 1e-9] f2(r_w) / r_w
//   E   = [d < eps] 1/2 k (d - eps)^2 + lam f0(r_w)
//   g   = [d < eps] k (d - eps) n + lam a1 w
//   H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T - sum_i free_i u_i u_i^T))
//   M   = a1 P0 + f2r w w^T,   H = H_n + lam M
// The curvature term vanishes on a face (two free axes), is the rod's barrel term on an edge (one) and the ball's at a corner (none); an axis with
// h_i = 0 is never free.  b0, n0 and lam are constants of the step, so H in x has the sphere's form.  The reverse step's un-projected operator
// (spd = 0) holds H_n exact; every projected mode holds [d < eps] k n n^T, the eigen-clamp of H_n in closed form (eigenvalue k along n, 0 along the
// free axes, k (d - eps) / rho < 0 on the rest).  H is 3 x 3 on the vertex's own diagonal block: no constraint slot, no row list, no change of a
// factorisation plan.  Nothing is stored per step.
// q is formed from the LOCAL difference y - b, which is exactly 0 along a free axis and a difference of neighbours elsewhere, never from x minus a
// rounded closest point in the world (DESIGN.md 2.10 on why the rod needed cap_point); the gap is sph_gap of that difference about the origin.
// sph_fric and sph_M are the spheres', with SphHead::dc the motion of the box's point.  Degenerate pairs: rho < 1e-12 (a vertex inside the core
// box, deeper than r) contributes nothing; rho0 < 1e-12 has no friction.
// The kernels are k_shape.hpp's with BoxShape below: one lane per VERTEX, the boxes in ascending j, the table by value in the kernel arguments (the
// matrices are uniform and load as scalars).  Launched only while boxes exist and k_box != 0.
#pragma once
#include "box_host.hpp"
#include "k_sphere.hpp"

// axis i of the matrix at r[0 .. 9) (row-major): its column i
TSL_DEV d3 box_axis(const double* r, int i) { return d3(r[i], r[3 + i], r[6 + i]); }

// the cheap part of the pair (vertex, box j): the sphere's head about the closest points, and on which faces, edges or corners they lie
struct BoxHead {
  SphHead h;            // q = R (y - b), q0 = R0 (y0 - b0), dc = (c - cp) + (R - R0) b0
  const double* row;    // the box's row of the table (uniform)
  d3 b0, Rb;            // local; R b0, the material point under the vertex about the centre of this step
  d3 xc, xpc;           // x - c, x_prev - cp
  unsigned fr, fr0;     // bit i: axis i free at x, at x_prev
};
// pose (c at row[oc], R at row[oc + 3]): b, the free bits, q = R (y - b), rho and the gap
TSL_DEV double box_gap(const double* row, int oc, const d3& x, d3& a, d3& b, unsigned& fr, d3& q, double& rho) {
  const double* R = row + oc + 3;
  const d3 u0 = box_axis(R, 0), u1 = box_axis(R, 1), u2 = box_axis(R, 2);
  a = x - d3(row[oc], row[oc + 1], row[oc + 2]);
  const d3 y(dot(u0, a), dot(u1, a), dot(u2, a));
  const d3 hh(row[BOX_H], row[BOX_H + 1], row[BOX_H + 2]);
  b = d3(fmin(fmax(y.x, -hh.x), hh.x), fmin(fmax(y.y, -hh.y), hh.y), fmin(fmax(y.z, -hh.z), hh.z));
  fr = (y.x > -hh.x && y.x < hh.x ? 1u : 0u) | (y.y > -hh.y && y.y < hh.y ? 2u : 0u) | (y.z > -hh.z && y.z < hh.z ? 4u : 0u);
  d3 ql;
  const double d = sph_gap(y - b, d3(0.0, 0.0, 0.0), row[BOX_RAD], ql, rho);
  q = (u0 * ql.x + u1 * ql.y) + u2 * ql.z;
  return d;
}
TSL_DEV BoxHead box_head(const BoxTable& S, int j, const d3& x, const d3& xp) {
  BoxHead c;
  const double* r = S.row[j];
  c.row = r;
  SphHead& h = c.h;
  h.mu = r[BOX_MU];
  d3 b;
  h.d = box_gap(r, BOX_C, x, c.xc, b, c.fr, h.q, h.rho); h.d0 = box_gap(r, BOX_CP, xp, c.xpc, c.b0, c.fr0, h.q0, h.rho0);
  c.Rb = (box_axis(r + BOX_R, 0) * c.b0.x + box_axis(r + BOX_R, 1) * c.b0.y) + box_axis(r + BOX_R, 2) * c.b0.z;
  const d3 R0b = (box_axis(r + BOX_R0, 0) * c.b0.x + box_axis(r + BOX_R0, 1) * c.b0.y) + box_axis(r + BOX_R0, 2) * c.b0.z;
  h.dc = d3(r[BOX_C] - r[BOX_CP], r[BOX_C + 1] - r[BOX_CP + 1], r[BOX_C + 2] - r[BOX_CP + 2]) + (c.Rb - R0b);
  h.ok = h.rho >= 1e-12;
  h.act = h.d < S.eps;
  h.pen = h.rho0 >= 1e-12 ? fmax(0.0, S.eps - h.d0) : 0.0;
  h.lam = (h.mu * S.k) * h.pen;
  return c;
}
// [d < eps]: the ball's normal block and, where exact, minus the curvature along the free axes
TSL_DEV void box_normal_block(const BoxHead& c, double k, double eps, int exact, d3& g, Sym3& H) {
  const SphHead& h = c.h;
  sph_normal_block(h, k, eps, exact, g, H);
  if (exact) {
    const double cr = k * (h.d - eps) / h.rho;
#pragma unroll
    for (int i = 0; i < 3; i++)
      if ((c.fr >> i) & 1u) {
        const d3 u = box_axis(c.row + BOX_R, i);
        H.xx -= cr * (u.x * u.x); H.xy -= cr * (u.x * u.y); H.xz -= cr * (u.x * u.z);
        H.yy -= cr * (u.y * u.y); H.yz -= cr * (u.y * u.z); H.zz -= cr * (u.z * u.z);
      }
  }
}
// H_n y, exact
TSL_DEV d3 box_Hn(const BoxHead& c, double k, double eps, const d3& y) {
  const SphHead& h = c.h;
  const d3 n = h.q / h.rho;
  const double ny = dot(n, y), cr = k * (h.d - eps) / h.rho;
  d3 t = y - n * ny;
#pragma unroll
  for (int i = 0; i < 3; i++) {   // (a select, no branch: the lanes of a wave lie on faces, edges and corners at once)
    const d3 u = box_axis(c.row + BOX_R, i);
    t = t - u * ((c.fr >> i) & 1u ? dot(u, y) : 0.0);
  }
  return n * (k * ny) + t * cr;
}
// The lagged terms applied to y (lam > 0), with B = a1 I + f2r w w^T,  z = J_n^T y = -((n0 . D) B y + D (n0 . B y)),
// G0 = P0 - sum_i free0_i u0_i u0_i^T,  Delta = sum_i free0_i (u_i - u0_i) u0_i^T (what a change of b0 costs):
//   X = lam (M y - G0 z / rho0) + [d0 < eps] mu k n0 (a1 w . y) + lam Delta^T M y = -(dg/dx_prev)^T y;   mz = -z
TSL_DEV d3 box_prev(const BoxHead& c, const SphFric& f, double k, double eps, const d3& y, d3& mz) {
  const SphHead& h = c.h;
  const d3 By = y * f.a + f.w * (f.f2r * dot(f.w, y));
  mz = By * dot(f.n0, f.D) + f.D * dot(f.n0, By);
  const d3 My = sph_M(f, y);
  d3 Gz = mz - f.n0 * dot(f.n0, mz), dl(0.0, 0.0, 0.0);
#pragma unroll
  for (int i = 0; i < 3; i++) {   // (selects, as in box_Hn)
    const bool on = (c.fr0 >> i) & 1u;
    const d3 u0 = box_axis(c.row + BOX_R0, i);
    Gz = Gz - u0 * (on ? dot(u0, mz) : 0.0);
    dl = dl + u0 * (on ? dot(box_axis(c.row + BOX_R, i) - u0, My) : 0.0);
  }
  const d3 X = ((My + dl) + Gz / h.rho0) * h.lam;
  return X + f.n0 * (h.d0 < eps ? (h.mu * k) * (f.a * dot(f.w, y)) : 0.0);
}

struct BoxShape {
  using Table = BoxTable;
  static constexpr int stride = 16, n_force = 6, n_grad = 14;
  static TSL_DEV void assemble(const Table& S, int j, const d3& x, const d3& xp, int exact, d3& g, Sym3& H) {
    const BoxHead c = box_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (!h.ok || (!h.act && !(h.lam > 0.0))) return;
    if (h.act) box_normal_block(c, S.k, S.eps, exact, g, H);
    if (h.lam > 0.0) sph_friction_block(h, sph_fric(h, x, xp, S.eh), g, H);
  }
  static TSL_DEV void energy(const Table& S, int j, const d3& x, const d3& xp, double& e) { sph_energy_pair(box_head(S, j, x, xp).h, S, x, xp, e); }
  // -(dg / dx_prev)^T p_v, the poses and previous poses of step s in the table
  static TSL_DEV void backprop(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, d3& acc) {
    const BoxHead c = box_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (!h.ok || !(h.lam > 0.0)) return;   // (lam > 0 implies d0 < eps and mu > 0)
    d3 mz;
    acc = acc + box_prev(c, sph_fric(h, x, xp, S.eh), S.k, S.eps, pv, mz);
  }
  // tsl_box_force: -g_v of box j, the force the box applies to the cloth, and -(x_v - c) x g_v, its torque about the box's centre, in the sign of
  // the force
  static TSL_DEV void force(const Table& S, int j, const d3& x, const d3& xp, double (&s)[6]) {
    const BoxHead c = box_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (h.ok && (h.act || h.lam > 0.0)) {
      const d3 g = sph_pair_g(h, S, x, xp);
      const d3 tq = cross(c.xc, g);
      s[0] = -g.x; s[1] = -g.y; s[2] = -g.z; s[3] = -tq.x; s[4] = -tq.y; s[5] = -tq.z;
    }
  }
  // tsl_box_grad: this reverse step's share of d(loss)/d(c_j) (3), d(loss)/d(theta_j) (3), d(loss)/d(cp_j) (3), d(loss)/d(theta_p_j) (3),
  // d(loss)/d(mu_j), d(loss)/d(r_j), each -(dg/d.)^T p_v, H_n exact; theta, theta_p: world-frame rotation vectors applied on the left
  static TSL_DEV void grad(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, double (&s)[14]) {
    const BoxHead c = box_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (h.ok && (h.act || h.pen > 0.0)) {
      d3 gc(0.0, 0.0, 0.0), gt(0.0, 0.0, 0.0);
      if (h.act) {
        // -(dg/dc)^T p = H_n p,  -(dg/dtheta)^T p = (x - c) x (H_n p) + p x g_n
        const d3 n = h.q / h.rho;
        gc = box_Hn(c, S.k, S.eps, pv);
        gt = cross(c.xc, gc) + cross(pv, n * (S.k * (h.d - S.eps)));
        s[13] = S.k * dot(n, pv);
      }
      if (h.pen > 0.0) {
        const SphFric f = sph_fric(h, x, xp, S.eh);
        const double paw = f.a * dot(f.w, pv);
        if (h.lam > 0.0) {
          // the material point R b0 rides on the pose of this step; x_prev - cp = R0 b0 + q0 on that of the last
          const d3 Mp = sph_M(f, pv) * h.lam;
          gc = gc + Mp; gt = gt + cross(c.Rb, Mp);
          d3 mz;
          const d3 X = box_prev(c, f, S.k, S.eps, pv, mz);
          const d3 gtp = (cross(h.q0, Mp) + cross(f.n0, mz) * h.lam) - cross(c.xpc, X);
          s[6] = -X.x; s[7] = -X.y; s[8] = -X.z; s[9] = gtp.x; s[10] = gtp.y; s[11] = gtp.z;
        }
        s[12] = -((S.k * h.pen) * paw);
        if (h.d0 < S.eps) {
#pragma clang fp contract(off)   // (the product rounded on its own: it is the one box_prev forms, not a part of an fma here)
          s[13] -= (h.mu * S.k) * paw;
        }
      }
      s[0] = gc.x; s[1] = gc.y; s[2] = gc.z; s[3] = gt.x; s[4] = gt.y; s[5] = gt.z;
    }
  }
};
