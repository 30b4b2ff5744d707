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
// One lane per VERTEX, the spheres in ascending j, the table by value in the kernel arguments.  A vertex with mask 0 leaves at once; a pair with
// d >= eps and lam = 0 leaves behind the two square roots rho, rho0.  No atomics, every sum in a fixed order: the same bits run to run.  Launched
// only while spheres exist and k_sphere != 0.  Frozen dofs follow the rule of every other term: the assembly adds to the unmasked gradient and
// matrix, k_mask_vec / k_mask_matrix behind it take the frozen entries out again.
#pragma once
#include "k_contact.hpp"
#include "k_handle.hpp"
#include "sphere_host.hpp"
#include "tsl_device.hpp"

struct SphereArgs {
  int NV;
  const unsigned char* mask;   // NV: bit j set: sphere j acts on the vertex
};

// the cheap part of the pair (vertex, sphere j): two square roots
struct SphHead {
  d3 q, q0, dc;   // x - c, x_prev - cp, c - cp
  double rho, rho0, d, d0, mu, pen, lam;
  bool ok, act;   // ok: rho >= 1e-12;  act: d < eps
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
  const double* t = S.sp[j];
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

// F[v] += g (where a gradient is asked for), diagonal block of v += H through diag_blk, as k_collider_assemble.  The upper triangle of H is formed
// and mirrored: the block is symmetric bit for bit.  exact (uniform): spd == 0, the curvature part of H_n is added; else it is left out.
__global__ void __launch_bounds__(256) k_sphere_assemble(SphereTable S, SphereArgs A, int exact, const double* __restrict__ pos, const double* __restrict__ prev,
                                                         const int* __restrict__ diag_blk, double* __restrict__ F, double* __restrict__ vals) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= A.NV) return;
  const unsigned m = A.mask[v];
  if (!m) return;
  const d3 x = ld3(pos, v), xp = ld3(prev, v);
  d3 g(0.0, 0.0, 0.0);
  double hxx = 0.0, hxy = 0.0, hxz = 0.0, hyy = 0.0, hyz = 0.0, hzz = 0.0;
  for (int j = 0; j < S.n; j++) {
    if (!((m >> j) & 1u)) continue;
    const SphHead h = sph_head(S, j, x, xp);
    if (!h.ok || (!h.act && !(h.lam > 0.0))) continue;
    if (h.act) {
      const d3 n = h.q / h.rho;
      const double kd = S.k * (h.d - S.eps);
      g = g + n * kd;
      hxx += S.k * (n.x * n.x); hxy += S.k * (n.x * n.y); hxz += S.k * (n.x * n.z);
      hyy += S.k * (n.y * n.y); hyz += S.k * (n.y * n.z); hzz += S.k * (n.z * n.z);
      if (exact) {
        const double cr = kd / h.rho;
        hxx += cr * (1.0 - n.x * n.x); hxy -= cr * (n.x * n.y); hxz -= cr * (n.x * n.z);
        hyy += cr * (1.0 - n.y * n.y); hyz -= cr * (n.y * n.z); hzz += cr * (1.0 - n.z * n.z);
      }
    }
    if (h.lam > 0.0) {
      const SphFric f = sph_fric(h, x, xp, S.eh);
      g = g + f.w * (h.lam * f.a);
      const d3& n0 = f.n0; const d3& w = f.w;
      hxx += h.lam * (f.a * (1.0 - n0.x * n0.x) + f.f2r * (w.x * w.x)); hxy += h.lam * (f.f2r * (w.x * w.y) - f.a * (n0.x * n0.y));
      hxz += h.lam * (f.f2r * (w.x * w.z) - f.a * (n0.x * n0.z)); hyy += h.lam * (f.a * (1.0 - n0.y * n0.y) + f.f2r * (w.y * w.y));
      hyz += h.lam * (f.f2r * (w.y * w.z) - f.a * (n0.y * n0.z)); hzz += h.lam * (f.a * (1.0 - n0.z * n0.z) + f.f2r * (w.z * w.z));
    }
  }
  if (F) st3(F, v, ld3(F, v) + g);
  const size_t base = (size_t)diag_blk[v];
  vals[base + 64 * 0] += hxx; vals[base + 64 * 1] += hxy; vals[base + 64 * 2] += hxz;
  vals[base + 64 * 3] += hxy; vals[base + 64 * 4] += hyy; vals[base + 64 * 5] += hyz;
  vals[base + 64 * 6] += hxz; vals[base + 64 * 7] += hyz; vals[base + 64 * 8] += hzz;
}

// one partial per workgroup (wg_join), behind the collider partials; k_energy_final adds them in its fixed order
__global__ void __launch_bounds__(256) k_sphere_energy(SphereTable S, SphereArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                       double* __restrict__ e_part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  if (m) {
    const d3 x = ld3(pos, v), xp = ld3(prev, v);
    for (int j = 0; j < S.n; j++) {
      if (!((m >> j) & 1u)) continue;
      const SphHead h = sph_head(S, j, x, xp);
      if (!h.ok || (!h.act && !(h.lam > 0.0))) continue;
      if (h.act) e[0] += 0.5 * S.k * (h.d - S.eps) * (h.d - S.eps);
      if (h.lam > 0.0) e[0] += h.lam * fr_f0(sph_fric(h, x, xp, S.eh).r, S.eh);
    }
  }
  wg_join<1>(e, e_part + blockIdx.x);
}

// p with its frozen dofs zeroed
TSL_DEV d3 sph_free_p(const int* __restrict__ frozen, const double* __restrict__ p, int v) {
  const int* __restrict__ fz = frozen + 3 * (size_t)v;
  const d3 pr = ld3(p, v);
  return d3(fz[0] ? 0.0 : pr.x, fz[1] ? 0.0 : pr.y, fz[2] ? 0.0 : pr.z);
}

// The reverse step: pos = x_s, prev = x_{s-1}, p the adjoint solution (its frozen dofs do not count), the centres and previous centres of step s in
// the table.  Into the vertex's own row of pos_grad[s-1], on free dofs:  += sum_j lam M p_v - L^T p_v = -(dg / dx_prev)^T p_v.  In front of k_adj_prev.
__global__ void __launch_bounds__(256) k_sphere_backprop(SphereTable S, SphereArgs A, const int* __restrict__ frozen, const double* __restrict__ pos,
                                                         const double* __restrict__ prev, const double* __restrict__ p, double* __restrict__ pg_prev) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= A.NV) return;
  const unsigned m = A.mask[v];
  if (!m) return;
  const int* __restrict__ fz = frozen + 3 * (size_t)v;
  const d3 pv = sph_free_p(frozen, p, v);
  const d3 x = ld3(pos, v), xp = ld3(prev, v);
  d3 acc(0.0, 0.0, 0.0);
  for (int j = 0; j < S.n; j++) {
    if (!((m >> j) & 1u)) continue;
    const SphHead h = sph_head(S, j, x, xp);
    if (!h.ok || !(h.lam > 0.0)) continue;   // (lam > 0 implies d0 < eps and mu > 0)
    acc = acc + sph_prev_term(h, sph_fric(h, x, xp, S.eh), S.k, S.eps, pv);
  }
  const d3 o = ld3(pg_prev, v);
  st3(pg_prev, v, d3(fz[0] ? o.x : o.x + acc.x, fz[1] ? o.y : o.y + acc.y, fz[2] ? o.z : o.z + acc.z));
}

// Read-outs.  A workgroup writes SPHERE_SLOTS partials, 8 per sphere; the spheres are joined one after the other (wg_join<8> / wg_join<3>), so that a
// lane holds the sums of one sphere at a time; k_sphere_join adds the partials in workgroup order.
#define SPHERE_SLOTS (8 * TSL_MAX_SPHERES)
// tsl_sphere_grad, slots 8 j ..: this reverse step's share of d(loss)/d(c_j) (3: (H_n + lam M) p_v, H_n exact), d(loss)/d(cp_j) (3: -(lam M p_v - L^T p_v)),
// d(loss)/d(mu_j) (-p_v . k max(0, eps - d0) a w), d(loss)/d(R_j) (-p_v . (-[d < eps] k n + [d0 < eps] mu k a w)), summed over the vertices.  Free dofs of p only.
__global__ void __launch_bounds__(256) k_sphere_grad(SphereTable S, SphereArgs A, const int* __restrict__ frozen, const double* __restrict__ pos,
                                                     const double* __restrict__ prev, const double* __restrict__ p, double* __restrict__ part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  d3 pv, x, xp;
  if (m) { pv = sph_free_p(frozen, p, v); x = ld3(pos, v); xp = ld3(prev, v); }
  for (int j = 0; j < S.n; j++) {   // (uniform)
    double s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = 0.0;
    if ((m >> j) & 1u) {
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
          if (h.d0 < S.eps) s[7] -= (h.mu * S.k) * paw;
        }
        s[0] = gc.x; s[1] = gc.y; s[2] = gc.z;
      }
    }
    wg_join<8>(s, part + (size_t)SPHERE_SLOTS * blockIdx.x + 8 * j);
    __syncthreads();   // (the LDS of wg_join is used again for the next sphere)
  }
}
// tsl_sphere_force, slots 8 j .. 8 j + 2: -sum_v g_v of sphere j, the net force the ball applies to the cloth (the sign of k_collider_force); frozen dofs are not
// masked
__global__ void __launch_bounds__(256) k_sphere_force(SphereTable S, SphereArgs A, const double* __restrict__ pos, const double* __restrict__ prev,
                                                      double* __restrict__ part) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m = v < A.NV ? A.mask[v] : 0u;
  d3 x, xp;
  if (m) { x = ld3(pos, v); xp = ld3(prev, v); }
  for (int j = 0; j < S.n; j++) {   // (uniform)
    double s[3] = {0.0, 0.0, 0.0};
    if ((m >> j) & 1u) {
      const SphHead h = sph_head(S, j, x, xp);
      if (h.ok && (h.act || h.lam > 0.0)) {
        d3 g(0.0, 0.0, 0.0);
        if (h.act) g = g + (h.q / h.rho) * (S.k * (h.d - S.eps));
        if (h.lam > 0.0) {
          const SphFric f = sph_fric(h, x, xp, S.eh);
          g = g + f.w * (h.lam * f.a);
        }
        s[0] = -g.x; s[1] = -g.y; s[2] = -g.z;
      }
    }
    wg_join<3>(s, part + (size_t)SPHERE_SLOTS * blockIdx.x + 8 * j);
    __syncthreads();
  }
}
// out[per j + i] = part[0][8 j + i] + part[1][8 j + i] + ..., in workgroup order, for j < n, i < per: one lane per slot
__global__ void k_sphere_join(int n_wg, int n, int per, const double* __restrict__ part, double* __restrict__ out) {
  const int q = threadIdx.x, j = q >> 3, i = q & 7;
  if (j >= n || i >= per) return;
  double t = 0.0;
  for (int w = 0; w < n_wg; w++) t += part[(size_t)SPHERE_SLOTS * w + q];
  out[per * j + i] = t;
}
