// Capsule colliders (tsl_set_capsules): capsule j is a solid rod with round ends and the cloth outside, endpoints a_j, b_j (may be
// set before every step), previous endpoints ap_j, bp_j (where the rod was at the start of the step), radius R_j and friction mu_j.  For vertex v
// (position x, start-of-step position x_prev) and capsule j, with k = "k_capsule", eps = eps_contact, eh = eps_v dt:
//   e  = b - a,    s  = (x - a) . e / (e . e),           t  = clamp(s, 0, 1),   in  = [0 < s < 1]
//   c  = a + t e,  q  = x - c,  rho = |q|,  n = q / rho,  d = rho - R,           u  = e / |e|
//   e0 = bp - ap,  s0 = (x_prev - ap) . e0 / (e0 . e0),  t0 = clamp(s0, 0, 1),  in0 = [0 < s0 < 1]
//   c0 = ap + t0 e0,  q0 = x_prev - c0,  rho0, n0, d0 = rho0 - R,                u0 = e0 / |e0|
//   lam = mu k max(0, eps - d0)  (the lagged normal force)
//   D   = (x - x_prev) - ((1 - t0)(a - ap) + t0 (b - bp))     the slip relative to the rod's material point at t0
//   P0 = I - n0 n0^T,  w = P0 D,  r = |w|,  a1 = f1(r),  f2r = [r > 1e-9] f2(r) / r
//   E   = [d < eps] 1/2 k (d - eps)^2 + lam f0(r)
//   g   = [d < eps] k (d - eps) n + lam a1 w
//   H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T - in u u^T))     exact: on the barrel the distance to a line has no curvature along it
//   M   = a1 P0 + f2r w w^T                                                  positive semi-definite
//   H   = H_n + lam M
// t0, n0 and lam are constants of the step, so H in x has the sphere's form.  The reverse step's un-projected operator (spd = 0) holds H_n exact;
// every projected mode (spd 1 and 2, with and without "spd_literal") holds [d < eps] k n n^T, the eigen-clamp of H_n in closed form (eigenvectors
// n, u, n x u with eigenvalues k, 0, k (d - eps) / rho < 0; on a cap the last one twice).  H is 3 x 3 on the vertex's own diagonal block: no
// constraint slot, no row list, no change of a factorisation plan.  Nothing is stored per step.
// The gap is sph_gap of k_sphere.hpp about the rounded closest point, corrected by the rounding error of that point (cap_gap); sph_fric and sph_M
// are the spheres', with SphHead::dc the motion of the rod's point.  Degenerate pairs: rho < 1e-12 contributes nothing; rho0 < 1e-12 has no
// friction.  Segments shorter than 1e-9 m never get here (capsule_host.hpp refuses them).
// The kernels are k_shape.hpp's with CapsuleShape below: one lane per VERTEX, the capsules in ascending j, the table by value in the kernel
// arguments; a pair with d >= eps and lam = 0 leaves behind the two heads (two square roots, four divisions).  The normal block, the friction
// block, the energy and the gradient of a pair are the spheres' (k_sphere.hpp), with the barrel term under CapHead::barrel.  Launched only while
// capsules exist and k_capsule != 0.
#pragma once
#include "capsule_host.hpp"
#include "k_sphere.hpp"

// the cheap part of the pair (vertex, capsule j): the sphere's head about the closest points, and where on the rod they lie
struct CapHead {
  SphHead h;         // q = x - c, q0 = x_prev - c0, dc = (1 - t0)(a - ap) + t0 (b - bp)
  d3 e, e0;          // b - a, bp - ap
  double ee, ee0;    // e . e, e0 . e0
  double t, t0, s0;
  bool in, in0;
  static constexpr bool barrel = true;
  TSL_DEV const SphHead& sph() const { return h; }
};
// The closest point c = a + t e as an unevaluated sum ch + cl: the product's rounding error by fma, the sum's by a two-sum.  A rounded c alone is
// off by half a last bit of |c| (1e-16 m for a rod of radius 1 m), which is 1e-12 of a penetration of 1e-4 m and shows in lam and in every entry
// scaled by it.  The gap about ch is sph_gap's; cl moves it by -n . cl (second order: 1e-32 m).
TSL_DEV void cap_point(const d3& a, const d3& e, double t, d3& ch, d3& cl) {
#pragma clang fp contract(off)
  const double px = e.x * t, py = e.y * t, pz = e.z * t;
  const double fx = fma(e.x, t, -px), fy = fma(e.y, t, -py), fz = fma(e.z, t, -pz);
  double sx, sy, sz, rx, ry, rz;
  sph_two_sum(a.x, px, sx, rx); sph_two_sum(a.y, py, sy, ry); sph_two_sum(a.z, pz, sz, rz);
  ch = d3(sx, sy, sz); cl = d3(rx + fx, ry + fy, rz + fz);
}
TSL_DEV double cap_gap(const d3& x, const d3& a, const d3& e, double t, double R, d3& q, double& rho) {
  d3 ch, cl;
  cap_point(a, e, t, ch, cl);
  const double d = sph_gap(x, ch, R, q, rho);
  return d - dot(q, cl) / rho;
}
TSL_DEV CapHead cap_head(const CapsuleTable& S, int j, const d3& x, const d3& xp) {
  CapHead c;
  const double* r = S.row[j];
  const d3 a(r[0], r[1], r[2]), b(r[3], r[4], r[5]), ap(r[6], r[7], r[8]), bp(r[9], r[10], r[11]);
  const double R = r[12];
  c.e = b - a; c.e0 = bp - ap;
  c.ee = dot(c.e, c.e); c.ee0 = dot(c.e0, c.e0);
  const double s = dot(x - a, c.e) / c.ee;
  c.s0 = dot(xp - ap, c.e0) / c.ee0;
  c.in = s > 0.0 && s < 1.0; c.in0 = c.s0 > 0.0 && c.s0 < 1.0;
  c.t = fmin(fmax(s, 0.0), 1.0); c.t0 = fmin(fmax(c.s0, 0.0), 1.0);
  SphHead& h = c.h;
  h.mu = r[13];
  h.dc = (a - ap) + (c.e - c.e0) * c.t0;
  h.d = cap_gap(x, a, c.e, c.t, R, h.q, h.rho); h.d0 = cap_gap(xp, ap, c.e0, c.t0, R, h.q0, h.rho0);
  h.ok = h.rho >= 1e-12;
  h.act = h.d < S.eps;
  h.pen = h.rho0 >= 1e-12 ? fmax(0.0, S.eps - h.d0) : 0.0;
  h.lam = (h.mu * S.k) * h.pen;
  return c;
}
// H_n y, exact
TSL_DEV d3 cap_Hn(const CapHead& c, double k, double eps, const d3& y) {
  const SphHead& h = c.h;
  const d3 n = h.q / h.rho;
  const double ny = dot(n, y), cr = k * (h.d - eps) / h.rho;
  d3 t = y - n * ny;
  if (c.in) t = t - c.e * (dot(c.e, y) / c.ee);
  return n * (k * ny) + t * cr;
}
// The lagged terms applied to y (lam > 0), with B = a1 I + f2r w w^T,  z = J_n^T y = -((n0 . D) B y + D (n0 . B y)),  G0 = I - n0 n0^T - in0 u0 u0^T:
//   X   = [d0 < eps] mu k n0 (a1 w . y) + lam (M y - G0 z / rho0)      the sphere's -(dg/dx_prev)^T y with G0 for P0
//   DMy = (e - e0) . M y                                               Delta . M y, what a change of t0 costs
//   t0z = -in0 e0 . z / (e0 . e0)                                      -tau0 . z
// so that  -(dg/dx_prev)^T y = X + lam tau0 DMy,
//          -(dg/dap)^T y = -(1 - t0) X + lam (dt0/dap DMy + n0 t0z),   dt0/dap = in0 (-q0 - (1 - s0) e0) / (e0 . e0),
//          -(dg/dbp)^T y = -t0 X       + lam (dt0/dbp DMy - n0 t0z),   dt0/dbp = in0 ( q0 - s0 e0) / (e0 . e0).
struct CapPrev {
  d3 X;
  double DMy, t0z;
};
TSL_DEV CapPrev cap_prev(const CapHead& c, const SphFric& f, double k, double eps, const d3& y) {
  const SphHead& h = c.h;
  CapPrev o;
  const d3 By = y * f.a + f.w * (f.f2r * dot(f.w, y));
  const d3 mz = By * dot(f.n0, f.D) + f.D * dot(f.n0, By);   // -z
  const double e0z = c.in0 ? dot(c.e0, mz) / c.ee0 : 0.0;
  const d3 Gz = (mz - f.n0 * dot(f.n0, mz)) - c.e0 * e0z;
  const d3 My = sph_M(f, y);
  o.X = (My + Gz / h.rho0) * h.lam;
  if (h.d0 < eps) o.X = o.X + f.n0 * ((h.mu * k) * (f.a * dot(f.w, y)));
  o.DMy = dot(c.e - c.e0, My);
  o.t0z = e0z;
  return o;
}

struct CapsuleShape {
  using Table = CapsuleTable;
  static constexpr int stride = 16, n_force = 6, n_grad = 14;
  static TSL_DEV void assemble(const Table& S, int j, const d3& x, const d3& xp, int exact, d3& g, Sym3& H) {
    sph_assemble_pair(cap_head(S, j, x, xp), S, x, xp, exact, g, H);
  }
  static TSL_DEV void energy(const Table& S, int j, const d3& x, const d3& xp, double& e) { sph_energy_pair(cap_head(S, j, x, xp).h, S, x, xp, e); }
  // -(dg / dx_prev)^T p_v, the endpoints and previous endpoints of step s in the table
  static TSL_DEV void backprop(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, d3& acc) {
    const CapHead c = cap_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (!h.ok || !(h.lam > 0.0)) return;   // (lam > 0 implies d0 < eps and mu > 0)
    const CapPrev o = cap_prev(c, sph_fric(h, x, xp, S.eh), S.k, S.eps, pv);
    acc = acc + o.X;
    if (c.in0) acc = acc + c.e0 * (h.lam * o.DMy / c.ee0);
  }
  // tsl_capsule_force: -g_v of capsule j, the force the rod applies to the cloth, and -(x_v - m) x g_v, its torque about the rod's midpoint
  // m = (a + b) / 2, in the sign of the force
  static TSL_DEV void force(const Table& S, int j, const d3& x, const d3& xp, double (&s)[6]) {
    const CapHead c = cap_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (h.ok && (h.act || h.lam > 0.0)) {
      const d3 g = sph_pair_g(h, S, x, xp);
      const double* r = S.row[j];
      const d3 arm = x - d3(0.5 * (r[0] + r[3]), 0.5 * (r[1] + r[4]), 0.5 * (r[2] + r[5]));
      const d3 tq = cross(arm, g);
      s[0] = -g.x; s[1] = -g.y; s[2] = -g.z; s[3] = -tq.x; s[4] = -tq.y; s[5] = -tq.z;
    }
  }
  // tsl_capsule_grad: this reverse step's share of d(loss)/d(a_j) (3), d(loss)/d(b_j) (3), d(loss)/d(ap_j) (3), d(loss)/d(bp_j) (3),
  // d(loss)/d(mu_j), d(loss)/d(R_j), each -(dg/d.)^T p_v, H_n exact
  static TSL_DEV void grad(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, double (&s)[14]) {
    const CapHead c = cap_head(S, j, x, xp);
    const SphHead& h = c.h;
    if (h.ok && (h.act || h.pen > 0.0)) {
      d3 ga(0.0, 0.0, 0.0), gb(0.0, 0.0, 0.0);
      if (h.act) {
        // -(dg/da)^T p = (1 - t) H_n p - phi' n (tau . p),  -(dg/db)^T p = t H_n p + phi' n (tau . p),  tau = in e / (e . e)
        const d3 Hp = cap_Hn(c, S.k, S.eps, pv);
        const d3 n = h.q / h.rho;
        const d3 tn = n * (c.in ? (S.k * (h.d - S.eps)) * (dot(c.e, pv) / c.ee) : 0.0);
        ga = Hp * (1.0 - c.t) - tn; gb = Hp * c.t + tn;
        s[13] = S.k * dot(n, pv);
      }
      if (h.pen > 0.0) {
        const SphFric f = sph_fric(h, x, xp, S.eh);
        const double paw = f.a * dot(f.w, pv);
        if (h.lam > 0.0) {
          const d3 Mp = sph_M(f, pv) * h.lam;
          ga = ga + Mp * (1.0 - c.t0); gb = gb + Mp * c.t0;
          const CapPrev o = cap_prev(c, f, S.k, S.eps, pv);
          d3 gap = -(o.X * (1.0 - c.t0)) + f.n0 * (h.lam * o.t0z), gbp = -(o.X * c.t0) - f.n0 * (h.lam * o.t0z);
          if (c.in0) {
            const double sc = h.lam * o.DMy / c.ee0;
            gap = gap - (h.q0 + c.e0 * (1.0 - c.s0)) * sc; gbp = gbp + (h.q0 - c.e0 * c.s0) * sc;
          }
          s[6] = gap.x; s[7] = gap.y; s[8] = gap.z; s[9] = gbp.x; s[10] = gbp.y; s[11] = gbp.z;
        }
        s[12] = -((S.k * h.pen) * paw);
        if (h.d0 < S.eps) {
#pragma clang fp contract(off)   // (the product rounded on its own: it is the one cap_prev forms, not a part of an fma here)
          s[13] -= (h.mu * S.k) * paw;
        }
      }
      s[0] = ga.x; s[1] = ga.y; s[2] = ga.z; s[3] = gb.x; s[4] = gb.y; s[5] = gb.z;
    }
  }
};
