// Sphere colliders (tsl_set_spheres): sphere j is a solid ball with the cloth outside, centre c_j (may be set before every step),
// previous centre cp_j (where the ball was at the start of the step), radius R_j and friction mu_j.  For vertex v (position x, start-of-step
// position x_prev) and sphere j, with k = "k_sphere", eps = eps_contact, eh = eps_v dt:
//   q  = x - c,       rho  = |q|,  n  = q / rho,   d  = rho - R
//   q0 = x_prev - cp, rho0 = |q0|, n0 = q0 / rho0, d0 = rho0 - R
//   lam = mu k max(0, eps - d0)  (the lagged normal force),  P0 = I - n0 n0^T,  D = (x - x_prev) - (c - cp),  w = P0 D,  r = |w|,  a = f1(r)
//   E   = [d < eps] 1/2 k (d - eps)^2 + lam f0(r)
//   g   = [d < eps] k (d - eps) n + lam a w
//   H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T))      exact; the second part is NEGATIVE in the tangent plane
//   M   = a P0 + [r > 1e-9] (f2 / r) w w^T                         positive semi-definite
//   H   = H_n + lam M
// with fr_f0 / fr_f1 / fr_f2 of k_contact.hpp.  The friction has no tangent basis: it is smooth in n0, and the slip is relative to the ball.
// The reverse step's un-projected operator (spd = 0) holds H_n exact; every projected mode (spd 1 and 2, with and without "spd_literal") holds
// [d < eps] k n n^T, the eigen-clamp of H_n in closed form (its eigenvectors are n and the tangent plane), and adds the same numbers.  H is 3 x 3
// on the vertex's own diagonal block: no constraint slot, no row list, no change of a factorisation plan.  Nothing is stored per step.
// Degenerate pairs: rho < 1e-12 (the vertex in the centre: no normal) contributes nothing; rho0 < 1e-12 has no friction.
// The kernels are k_shape.hpp's with SphereShape below: one lane per VERTEX, the spheres in ascending j, the table by value in the kernel
// arguments; a pair with d >= eps and lam = 0 leaves behind the two square roots rho, rho0.  Launched only while spheres exist and k_sphere != 0.
// The blocks that a rod shares (sph_normal_block, sph_friction_block, sph_pair_g and the pair functions built on them) take the pair's head as a
// template argument: Head::barrel tells the capsule's (k_capsule.hpp), whose additions are compiled into its own instances only.
#pragma once
#include "k_contact.hpp"
#include "k_shape.hpp"
#include "sphere_host.hpp"

// the cheap part of the pair (vertex, sphere j): two square roots
struct SphHead {
  d3 q, q0, dc;   // x - c, x_prev - cp, c - cp
  double rho, rho0, d, d0, mu, pen, lam;
  bool ok, act;   // ok: rho >= 1e-12;  act: d < eps
  static constexpr bool barrel = false;
  TSL_DEV const SphHead& sph() const { return *this; }
};
// The gap |x - c| - R without its cancellations: a ball of radius 1e4 m (a floor in all but name) leaves |x - c| - R with the last bit of 1e4,
// 2e-12 m, where the gap itself is 1e-6 m, and the line search of a step then compares energies that carry this noise.  x - c = s + e exactly
// (two-sum per component); |s|^2 - R^2 as an unevaluated sum hi + lo (exact products by fma, two-sums in between); the gap is
// (hi + lo + 2 s . e) / (|q| + R).  q and rho come out rounded as usual: they only scale the result.  Nothing here may be contracted into an fma
// that the text does not write.
TSL_DEV void sph_two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
TSL_DEV double sph_gap(const d3& x, const d3& c, double R, d3& q, double& rho) {
#pragma clang fp contract(off)   // (a product fused into the sum behind it would not be the rounded product whose error the fma recovers)
  double sx, sy, sz, ex, ey, ez;
  sph_two_sum(x.x, -c.x, sx, ex); sph_two_sum(x.y, -c.y, sy, ey); sph_two_sum(x.z, -c.z, sz, ez);
  q = d3(sx, sy, sz);
  const double px = sx * sx, py = sy * sy, pz = sz * sz, rr = R * R;
  double lo = ((fma(sx, sx, -px) + fma(sy, sy, -py)) + fma(sz, sz, -pz)) - fma(R, R, -rr);
  double hi, e;
  sph_two_sum(px, py, hi, e); lo += e;
  sph_two_sum(hi, pz, hi, e); lo += e;
  rho = sqrt(hi);
  sph_two_sum(hi, -rr, hi, e); lo += e;
  lo += 2.0 * ((sx * ex + sy * ey) + sz * ez);
  return (hi + lo) / (rho + R);
}
TSL_DEV SphHead sph_head(const SphereTable& S, int j, const d3& x, const d3& xp) {
  SphHead h;
  const double* t = S.row[j];
  const d3 c(t[0], t[1], t[2]), cp(t[3], t[4], t[5]);
  h.mu = t[7];
  h.dc = c - cp;
  h.d = sph_gap(x, c, t[6], h.q, h.rho); h.d0 = sph_gap(xp, cp, t[6], h.q0, h.rho0);
  h.ok = h.rho >= 1e-12;
  h.act = h.d < S.eps;
  h.pen = h.rho0 >= 1e-12 ? fmax(0.0, S.eps - h.d0) : 0.0;
  h.lam = (h.mu * S.k) * h.pen;
  return h;
}
// the friction part, asked for only where pen > 0 (hence rho0 >= 1e-12)
struct SphFric {
  d3 n0, D, w;
  double r, a, f2r;   // f2r = [r > 1e-9] f2 / r
};
TSL_DEV SphFric sph_fric(const SphHead& h, const d3& x, const d3& xp, double eh) {
  SphFric f;
  f.n0 = h.q0 / h.rho0;
  f.D = (x - xp) - h.dc;
  f.w = f.D - f.n0 * dot(f.n0, f.D);
  f.r = sqrt(dot(f.w, f.w));
  f.a = fr_f1(f.r, eh);
  f.f2r = f.r > 1e-9 ? fr_f2(f.r, eh) / f.r : 0.0;
  return f;
}
// M y = a (y - n0 (n0 . y)) + f2r w (w . y)
TSL_DEV d3 sph_M(const SphFric& f, const d3& y) { return (y - f.n0 * dot(f.n0, y)) * f.a + f.w * (f.f2r * dot(f.w, y)); }
// H_n y, exact
TSL_DEV d3 sph_Hn(const SphHead& h, double k, double eps, const d3& y) {
  const d3 n = h.q / h.rho;
  const double ny = dot(n, y), cr = k * (h.d - eps) / h.rho;
  return n * (k * ny) + (y - n * ny) * cr;
}
// -(dg/dx_prev)^T y = lam M y - L^T y,  L = -[d0 < eps] mu k (a w) n0^T + lam J_n P0 / rho0,  J_n = -B ((n0 . D) I + n0 D^T),
// B = a I + f2r w w^T:   L^T y = -[d0 < eps] mu k (a w . y) n0 - (lam / rho0) P0 ((n0 . D) B y + D (n0 . B y))
TSL_DEV d3 sph_prev_term(const SphHead& h, const SphFric& f, double k, double eps, const d3& y) {
  const d3 By = y * f.a + f.w * (f.f2r * dot(f.w, y));
  const d3 z = By * dot(f.n0, f.D) + f.D * dot(f.n0, By);
  const d3 Pz = z - f.n0 * dot(f.n0, z);
  d3 Lty = Pz * (-(h.lam / h.rho0));
  if (h.d0 < eps) Lty = Lty - f.n0 * ((h.mu * k) * (f.a * dot(f.w, y)));
  return sph_M(f, y) * h.lam - Lty;
}

// [d < eps]: g += k (d - eps) n, H += k n n^T and, where exact, the curvature part of H_n (on a barrel without its part along the rod)
template <class Head>
TSL_DEV void sph_normal_block(const Head& c, double k, double eps, int exact, d3& g, Sym3& H) {
  const SphHead& h = c.sph();
  const d3 n = h.q / h.rho;
  const double kd = k * (h.d - eps);
  g = g + n * kd;
  H.xx += k * (n.x * n.x); H.xy += k * (n.x * n.y); H.xz += k * (n.x * n.z);
  H.yy += k * (n.y * n.y); H.yz += k * (n.y * n.z); H.zz += k * (n.z * n.z);
  if (exact) {
    const double cr = kd / h.rho;
    if constexpr (Head::barrel) {
      const double uu = c.in ? 1.0 / c.ee : 0.0;
      const d3& e = c.e;
      H.xx += cr * (1.0 - n.x * n.x - uu * (e.x * e.x)); H.xy -= cr * (n.x * n.y + uu * (e.x * e.y)); H.xz -= cr * (n.x * n.z + uu * (e.x * e.z));
      H.yy += cr * (1.0 - n.y * n.y - uu * (e.y * e.y)); H.yz -= cr * (n.y * n.z + uu * (e.y * e.z)); H.zz += cr * (1.0 - n.z * n.z - uu * (e.z * e.z));
    } else {
      H.xx += cr * (1.0 - n.x * n.x); H.xy -= cr * (n.x * n.y); H.xz -= cr * (n.x * n.z);
      H.yy += cr * (1.0 - n.y * n.y); H.yz -= cr * (n.y * n.z); H.zz += cr * (1.0 - n.z * n.z);
    }
  }
}
// [lam > 0]: g += lam a w, H += lam M
TSL_DEV void sph_friction_block(const SphHead& h, const SphFric& f, d3& g, Sym3& H) {
  g = g + f.w * (h.lam * f.a);
  const d3& n0 = f.n0; const d3& w = f.w;
  H.xx += h.lam * (f.a * (1.0 - n0.x * n0.x) + f.f2r * (w.x * w.x)); H.xy += h.lam * (f.f2r * (w.x * w.y) - f.a * (n0.x * n0.y));
  H.xz += h.lam * (f.f2r * (w.x * w.z) - f.a * (n0.x * n0.z)); H.yy += h.lam * (f.a * (1.0 - n0.y * n0.y) + f.f2r * (w.y * w.y));
  H.yz += h.lam * (f.f2r * (w.y * w.z) - f.a * (n0.y * n0.z)); H.zz += h.lam * (f.a * (1.0 - n0.z * n0.z) + f.f2r * (w.z * w.z));
}
// the pair functions of a Shape (k_shape.hpp) that a ball and a rod share, on the pair's head; S: the kind's table, for k, eps, eh
template <class Head, class Tab>
TSL_DEV void sph_assemble_pair(const Head& c, const Tab& S, const d3& x, const d3& xp, int exact, d3& g, Sym3& H) {
  const SphHead& h = c.sph();
  if (!h.ok || (!h.act && !(h.lam > 0.0))) return;
  if (h.act) sph_normal_block(c, S.k, S.eps, exact, g, H);
  if (h.lam > 0.0) sph_friction_block(h, sph_fric(h, x, xp, S.eh), g, H);
}
template <class Tab>
TSL_DEV void sph_energy_pair(const SphHead& h, const Tab& S, const d3& x, const d3& xp, double& e) {
  if (!h.ok || (!h.act && !(h.lam > 0.0))) return;
  if (h.act) e += 0.5 * S.k * (h.d - S.eps) * (h.d - S.eps);
  if (h.lam > 0.0) e += h.lam * fr_f0(sph_fric(h, x, xp, S.eh).r, S.eh);
}
// the pair's gradient g, asked for where h.ok && (h.act || h.lam > 0)
template <class Tab>
TSL_DEV d3 sph_pair_g(const SphHead& h, const Tab& S, const d3& x, const d3& xp) {
  d3 g(0.0, 0.0, 0.0);
  if (h.act) g = g + (h.q / h.rho) * (S.k * (h.d - S.eps));
  if (h.lam > 0.0) {
    const SphFric f = sph_fric(h, x, xp, S.eh);
    g = g + f.w * (h.lam * f.a);
  }
  return g;
}

struct SphereShape {
  using Table = SphereTable;
  static constexpr int stride = 8, n_force = 3, n_grad = 8;
  static TSL_DEV void assemble(const Table& S, int j, const d3& x, const d3& xp, int exact, d3& g, Sym3& H) {
    sph_assemble_pair(sph_head(S, j, x, xp), S, x, xp, exact, g, H);
  }
  static TSL_DEV void energy(const Table& S, int j, const d3& x, const d3& xp, double& e) { sph_energy_pair(sph_head(S, j, x, xp), S, x, xp, e); }
  // lam M p_v - L^T p_v = -(dg / dx_prev)^T p_v, the centres and previous centres of step s in the table
  static TSL_DEV void backprop(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, d3& acc) {
    const SphHead h = sph_head(S, j, x, xp);
    if (!h.ok || !(h.lam > 0.0)) return;   // (lam > 0 implies d0 < eps and mu > 0)
    acc = acc + sph_prev_term(h, sph_fric(h, x, xp, S.eh), S.k, S.eps, pv);
  }
  // tsl_sphere_force: -g_v of sphere j, the force the ball applies to the cloth
  static TSL_DEV void force(const Table& S, int j, const d3& x, const d3& xp, double (&s)[3]) {
    const SphHead h = sph_head(S, j, x, xp);
    if (h.ok && (h.act || h.lam > 0.0)) {
      const d3 g = sph_pair_g(h, S, x, xp);
      s[0] = -g.x; s[1] = -g.y; s[2] = -g.z;
    }
  }
  // tsl_sphere_grad: this reverse step's share of d(loss)/d(c_j) (3: (H_n + lam M) p_v, H_n exact), d(loss)/d(cp_j) (3: -(lam M p_v - L^T p_v)),
  // d(loss)/d(mu_j) (-p_v . k max(0, eps - d0) a w), d(loss)/d(R_j) (-p_v . (-[d < eps] k n + [d0 < eps] mu k a w))
  static TSL_DEV void grad(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, double (&s)[8]) {
    const SphHead h = sph_head(S, j, x, xp);
    if (h.ok && (h.act || h.pen > 0.0)) {
      d3 gc(0.0, 0.0, 0.0);
      if (h.act) {
        gc = sph_Hn(h, S.k, S.eps, pv);
        s[7] = S.k * dot(h.q, pv) / h.rho;
      }
      if (h.pen > 0.0) {
        const SphFric f = sph_fric(h, x, xp, S.eh);
        const double paw = f.a * dot(f.w, pv);
        if (h.lam > 0.0) {
          gc = gc + sph_M(f, pv) * h.lam;
          const d3 gp = sph_prev_term(h, f, S.k, S.eps, pv);
          s[3] = -gp.x; s[4] = -gp.y; s[5] = -gp.z;
        }
        s[6] = -((S.k * h.pen) * paw);
        if (h.d0 < S.eps) {
#pragma clang fp contract(off)   // (the product rounded on its own: it is the one sph_prev_term forms, not a part of an fma here)
          s[7] -= (h.mu * S.k) * paw;
        }
      }
      s[0] = gc.x; s[1] = gc.y; s[2] = gc.z;
    }
  }
};
