// Sampled distance-field colliders (tsl_set_sdfs): field j is the solid {phi < r} with the cloth outside, phi the tensor-product
// uniform cubic B-spline (C2) over n0 x n1 x n2 samples with spacing h and origin o in the field's own frame -- any solid, concave ones included: a
// mould, a bowl, a ring.  Centre c and rotation matrix R (may be set before every step), previous pose cp, R0 (where the field was at the start of
// the step), offset r, friction mu.  For a local point y:
//   t = (y - o) / h,  i_a = floor(t_a),  f_a = t_a - i_a,   valid  <=>  1 <= t_a < n_a - 2 for a = 0, 1, 2   (tested in double, NaN fails, before
//   any conversion to an integer)
//   phi(y) = sum_{a,b,c in 0..3} B_a(f_0) B_b(f_1) B_c(f_2) s[i_0-1+a, i_1-1+b, i_2-1+c]
//   B_0 = (1-f)^3/6,  B_1 = (3f^3 - 6f^2 + 4)/6,  B_2 = (-3f^3 + 3f^2 + 3f + 1)/6,  B_3 = f^3/6
//   grad phi: one factor B' and 1/h;   Hess phi: B'' or B'B' and 1/h^2
// The samples are the control values: a sampled linear field is reproduced exactly, a constant added to the samples is added to phi, a curved field
// is smoothed by about h^2/6 times its Laplacian (no prefilter).  For vertex v (position x, start-of-step position x_prev) and field j, with
// k = "k_sdf", eps = eps_contact, eh = eps_v dt:
//   y  = R^T (x - c),        d  = phi(y) - r,    m  = R grad phi(y)   (not normalised: the energy is a function of phi itself)
//   y0 = R0^T (x_prev - cp), d0 = phi(y0) - r,   s0 = |grad phi(y0)|,  n0 = R0 grad phi(y0) / s0
//   lam = [y0 valid][s0 >= 1e-12] mu k max(0, eps - d0)
//   D   = (x - c) - R y0 = (x - x_prev) - dc,  dc = (c - cp) + (R - R0) y0     the slip relative to the field's material point under the vertex
//   P0 = I - n0 n0^T,  w = P0 D,  r_w = |w|,  a1 = f1(r_w),  f2r = [r_w > 1e-9] f2(r_w) / r_w,  B = a1 I + f2r w w^T,  M = a1 P0 + f2r w w^T
//   E   = [y valid][d < eps] 1/2 k (d - eps)^2 + lam f0(r_w)
//   g   = [y valid][d < eps] k (d - eps) m + lam a1 w
//   H_n = [y valid][d < eps] k (m m^T + (d - eps) R Hess phi(y) R^T)     exact, spd = 0
//         [y valid][d < eps] k m m^T                                     every projected mode and spd_literal
//   H   = H_n + lam M
// The projected modes hold the Gauss-Newton part: positive semi-definite, but NOT the eigen-clamp of H_n -- the second-derivative matrix of a general
// field has no closed-form clamp worth its cost in a 3 x 3 block.  Outside the valid region a pair contributes nothing: at x no normal term, at
// x_prev no friction.  H is 3 x 3 on the vertex's own diagonal block: no constraint slot, no row list, no plan change, nothing stored per step.
// The reverse step, with z = -((n0 . D) B p + D (n0 . B p)):
//   X = -(dg/dx_prev)^T p = lam (R0 R^T M p - R0 Hess phi(y0) R0^T P0 z / s0) + [d0 < eps] mu k s0 n0 (a1 w . p)
// The sampler gathers 64 samples per point and never holds them at once: each row of four along the contiguous axis is reduced as it is loaded,
// then the rows of a slab, then the slabs, into at most ten running sums; index arithmetic in size_t; every sum in a fixed order.  It is a template
// on the derivative order, and a kernel compiles the cheapest variant it can do with: the energy takes the value at y, the projected assembly value
// and gradient, the exact assembly (exact is uniform) and the gradient read-out the Hessian; the reverse step samples at y0 only.
// sph_fric, sph_M, sph_friction_block and Sym3 are the spheres', as for BoxShape; SphHead::q holds m with rho = 1, q0 = R0 grad phi(y0), rho0 = s0.
// The kernels are k_shape.hpp's with SdfShape below.  Launched only while fields exist and k_sdf != 0.
#pragma once
#include "k_box.hpp"
#include "sdf_host.hpp"

// the four weights of one axis and, as asked for, their first and second derivatives in f
template <int ORD>
struct SdfAxis {
  double w[4], d1[ORD >= 1 ? 4 : 1], d2[ORD >= 2 ? 4 : 1];
  TSL_DEV explicit SdfAxis(double f) {
    const double g = 1.0 - f, f2 = f * f, g2 = g * g;
    w[0] = g2 * g * (1.0 / 6.0); w[1] = ((3.0 * f - 6.0) * f2 + 4.0) * (1.0 / 6.0);
    w[2] = (((-3.0 * f + 3.0) * f + 3.0) * f + 1.0) * (1.0 / 6.0); w[3] = f2 * f * (1.0 / 6.0);
    if constexpr (ORD >= 1) { d1[0] = -0.5 * g2; d1[1] = (1.5 * f - 2.0) * f; d1[2] = (-1.5 * f + 1.0) * f + 0.5; d1[3] = 0.5 * f2; }
    if constexpr (ORD >= 2) { d2[0] = g; d2[1] = 3.0 * f - 2.0; d2[2] = -3.0 * f + 1.0; d2[3] = f; }
  }
};
TSL_DEV double sdf_dot4(const double (&w)[4], double s0, double s1, double s2, double s3) { return ((w[0] * s0 + w[1] * s1) + w[2] * s2) + w[3] * s3; }

// phi (ORD 0), grad phi (ORD >= 1) and Hess phi (ORD 2) of field j at the local point y; false, and nothing written, outside the valid region
template <int ORD>
TSL_DEV bool sdf_sample(const SdfTable& S, int j, const d3& y, double& v, d3& g, Sym3& H) {
  const double* r = S.row[j];
  const double hh = r[SDF_H];
  const double t0 = (y.x - r[SDF_O]) / hh, t1 = (y.y - r[SDF_O + 1]) / hh, t2 = (y.z - r[SDF_O + 2]) / hh;
  const int n0 = S.dim[j][0], n1 = S.dim[j][1], n2 = S.dim[j][2];
  if (!(t0 >= 1.0 && t0 < (double)(n0 - 2) && t1 >= 1.0 && t1 < (double)(n1 - 2) && t2 >= 1.0 && t2 < (double)(n2 - 2))) return false;
  const double fl0 = floor(t0), fl1 = floor(t1), fl2 = floor(t2);
  const SdfAxis<ORD> A(t0 - fl0), B(t1 - fl1), C(t2 - fl2);
  // sample (i0 - 1, i1 - 1, i2 - 1): 0 <= i_a - 1 and i_a + 2 <= n_a - 1 by the test above
  const size_t N1 = (size_t)n1, N2 = (size_t)n2;
  const double* __restrict__ base = S.smp + (S.off[j] + ((((size_t)fl0 - 1) * N1 + ((size_t)fl1 - 1)) * N2 + ((size_t)fl2 - 1)));
  double p = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;
#pragma unroll
  for (int a = 0; a < 4; a++) {
    double sv = 0.0, s1 = 0.0, s2 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;   // the slab: value, d/d1, d/d2, d2/d1 d1, d2/d1 d2, d2/d2 d2
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const double* __restrict__ q = base + ((size_t)a * N1 + (size_t)b) * N2;
      const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      const double r0 = sdf_dot4(C.w, q0, q1, q2, q3);
      sv += B.w[b] * r0;
      if constexpr (ORD >= 1) {
        const double r1 = sdf_dot4(C.d1, q0, q1, q2, q3);
        s1 += B.d1[b] * r0; s2 += B.w[b] * r1;
        if constexpr (ORD >= 2) {
          s11 += B.d2[b] * r0; s12 += B.d1[b] * r1; s22 += B.w[b] * sdf_dot4(C.d2, q0, q1, q2, q3);
        }
      }
    }
    p += A.w[a] * sv;
    if constexpr (ORD >= 1) { g0 += A.d1[a] * sv; g1 += A.w[a] * s1; g2 += A.w[a] * s2; }
    if constexpr (ORD >= 2) { h00 += A.d2[a] * sv; h01 += A.d1[a] * s1; h02 += A.d1[a] * s2; h11 += A.w[a] * s11; h12 += A.w[a] * s12; h22 += A.w[a] * s22; }
  }
  v = p;
  if constexpr (ORD >= 1) g = d3(g0 / hh, g1 / hh, g2 / hh);
  if constexpr (ORD >= 2) {
    const double ih2 = 1.0 / (hh * hh);
    H.xx = h00 * ih2; H.xy = h01 * ih2; H.xz = h02 * ih2; H.yy = h11 * ih2; H.yz = h12 * ih2; H.zz = h22 * ih2;
  }
  return true;
}

// R a and R^T a of the matrix at r[0 .. 9) (row-major)
TSL_DEV d3 sdf_R(const double* r, const d3& a) { return (box_axis(r, 0) * a.x + box_axis(r, 1) * a.y) + box_axis(r, 2) * a.z; }
TSL_DEV d3 sdf_Rt(const double* r, const d3& a) { return d3(dot(box_axis(r, 0), a), dot(box_axis(r, 1), a), dot(box_axis(r, 2), a)); }
TSL_DEV d3 sym_mul(const Sym3& H, const d3& a) {
  return d3((H.xx * a.x + H.xy * a.y) + H.xz * a.z, (H.xy * a.x + H.yy * a.y) + H.yz * a.z, (H.xz * a.x + H.yz * a.y) + H.zz * a.z);
}
// R H R^T y for the local symmetric H
TSL_DEV d3 sdf_RHRt(const double* r, const Sym3& H, const d3& y) { return sdf_R(r, sym_mul(H, sdf_Rt(r, y))); }

// The pair at x: h.act = [y valid][d < eps], h.d, h.q = m (h.rho = 1, so that the spheres' q / rho is m), xc = x - c, Hl = Hess phi(y) (ORD 2)
template <int ORD>
TSL_DEV void sdf_here(const SdfTable& S, int j, const d3& x, SphHead& h, d3& xc, Sym3& Hl) {
  const double* r = S.row[j];
  xc = x - d3(r[SDF_C], r[SDF_C + 1], r[SDF_C + 2]);
  double v = 0.0;
  d3 gl;
  const bool val = sdf_sample<ORD>(S, j, sdf_Rt(r + SDF_R, xc), v, gl, Hl);
  h.ok = true;
  h.rho = 1.0;
  h.d = v - r[SDF_OFF];
  h.act = val && h.d < S.eps;
  if constexpr (ORD >= 1) h.q = sdf_R(r + SDF_R, gl);
}
// The lagged part, at x_prev: h.d0 (+inf where y0 is not valid, so that [d0 < eps] is false), h.q0 = R0 grad phi(y0) = s0 n0, h.rho0 = s0, h.pen,
// h.lam, h.dc; the local point, the material point about the centre of this step, x_prev - cp, and Hess phi(y0) (ORD 2)
struct SdfLag {
  d3 y0, Ry0, xpc;
  Sym3 H0;
};
template <int ORD>
TSL_DEV void sdf_lag(const SdfTable& S, int j, const d3& xp, SphHead& h, SdfLag& L) {
  const double* r = S.row[j];
  L.xpc = xp - d3(r[SDF_CP], r[SDF_CP + 1], r[SDF_CP + 2]);
  L.y0 = sdf_Rt(r + SDF_R0, L.xpc);
  double v = 0.0;
  d3 gl;
  const bool val0 = sdf_sample<ORD>(S, j, L.y0, v, gl, L.H0);
  h.mu = r[SDF_MU];
  h.q0 = sdf_R(r + SDF_R0, gl);
  h.rho0 = sqrt(dot(h.q0, h.q0));
  h.d0 = val0 ? v - r[SDF_OFF] : __builtin_inf();
  h.pen = val0 && h.rho0 >= 1e-12 ? fmax(0.0, S.eps - h.d0) : 0.0;
  h.lam = (h.mu * S.k) * h.pen;
  L.Ry0 = sdf_R(r + SDF_R, L.y0);
  h.dc = d3(r[SDF_C] - r[SDF_CP], r[SDF_C + 1] - r[SDF_CP + 1], r[SDF_C + 2] - r[SDF_CP + 2]) + (L.Ry0 - sdf_R(r + SDF_R0, L.y0));
}
// the lagged part switched off (mu = 0 where only lam counts: no sample at x_prev)
TSL_DEV void sdf_no_lag(SphHead& h) { h.mu = 0.0; h.pen = 0.0; h.lam = 0.0; h.d0 = __builtin_inf(); h.rho0 = 0.0; }

// The lagged terms applied to y (lam > 0):  X = lam (R0 R^T M y - R0 Hess phi(y0) R0^T P0 z / s0) + [d0 < eps] mu k s0 n0 (a1 w . y);   mz = -z
TSL_DEV d3 sdf_prev(const double* r, const SphHead& h, const SdfLag& L, const SphFric& f, double k, double eps, const d3& y, d3& mz) {
  const d3 By = y * f.a + f.w * (f.f2r * dot(f.w, y));
  mz = By * dot(f.n0, f.D) + f.D * dot(f.n0, By);
  const d3 My = sph_M(f, y);
  const d3 Pz = mz - f.n0 * dot(f.n0, mz);
  const d3 X = (sdf_R(r + SDF_R0, sdf_Rt(r + SDF_R, My)) + sdf_RHRt(r + SDF_R0, L.H0, Pz) / h.rho0) * h.lam;
  return X + h.q0 * (h.d0 < eps ? (h.mu * k) * (f.a * dot(f.w, y)) : 0.0);
}

struct SdfShape {
  using Table = SdfTable;
  static constexpr int stride = 16, n_force = 6, n_grad = 14;
  template <int ORD>
  static TSL_DEV void assemble_ord(const Table& S, int j, const d3& x, const d3& xp, d3& g, Sym3& H) {
    const double* r = S.row[j];
    SphHead h;
    d3 xc;
    Sym3 Hl;
    sdf_here<ORD>(S, j, x, h, xc, Hl);
    if (h.act) {
      const d3& m = h.q;
      const double kd = S.k * (h.d - S.eps);
      g = g + m * kd;
      H.xx += S.k * (m.x * m.x); H.xy += S.k * (m.x * m.y); H.xz += S.k * (m.x * m.z);
      H.yy += S.k * (m.y * m.y); H.yz += S.k * (m.y * m.z); H.zz += S.k * (m.z * m.z);
      if constexpr (ORD >= 2) {
        // kd R Hess phi R^T, its upper triangle from the columns T_i = R Hess phi e_i
        const double* R = r + SDF_R;
        const d3 T0 = sdf_R(R, d3(Hl.xx, Hl.xy, Hl.xz)), T1 = sdf_R(R, d3(Hl.xy, Hl.yy, Hl.yz)), T2 = sdf_R(R, d3(Hl.xz, Hl.yz, Hl.zz));
        const d3 R0r(R[0], R[1], R[2]), R1r(R[3], R[4], R[5]), R2r(R[6], R[7], R[8]);   // rows of R
        const d3 W0(T0.x, T1.x, T2.x), W1(T0.y, T1.y, T2.y), W2(T0.z, T1.z, T2.z);      // rows of R Hess phi
        H.xx += kd * dot(W0, R0r); H.xy += kd * dot(W0, R1r); H.xz += kd * dot(W0, R2r);
        H.yy += kd * dot(W1, R1r); H.yz += kd * dot(W1, R2r); H.zz += kd * dot(W2, R2r);
      }
    }
    if (r[SDF_MU] > 0.0) {   // (uniform)
      SdfLag L;
      sdf_lag<1>(S, j, xp, h, L);
      if (h.lam > 0.0) sph_friction_block(h, sph_fric(h, x, xp, S.eh), g, H);
    }
  }
  static TSL_DEV void assemble(const Table& S, int j, const d3& x, const d3& xp, int exact, d3& g, Sym3& H) {
    if (exact) assemble_ord<2>(S, j, x, xp, g, H);   // (uniform)
    else assemble_ord<1>(S, j, x, xp, g, H);
  }
  static TSL_DEV void energy(const Table& S, int j, const d3& x, const d3& xp, double& e) {
    SphHead h;
    d3 xc;
    Sym3 Hl;
    sdf_here<0>(S, j, x, h, xc, Hl);
    if (S.row[j][SDF_MU] > 0.0) { SdfLag L; sdf_lag<1>(S, j, xp, h, L); }
    else sdf_no_lag(h);
    sph_energy_pair(h, S, x, xp, e);
  }
  // -(dg / dx_prev)^T p_v, the poses and previous poses of step s in the table: nothing of phi at y enters
  static TSL_DEV void backprop(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, d3& acc) {
    if (!(S.row[j][SDF_MU] > 0.0)) return;   // (uniform)
    SphHead h;
    SdfLag L;
    sdf_lag<2>(S, j, xp, h, L);
    if (!(h.lam > 0.0)) return;   // (lam > 0 implies y0 valid, d0 < eps and mu > 0)
    d3 mz;
    acc = acc + sdf_prev(S.row[j], h, L, sph_fric(h, x, xp, S.eh), S.k, S.eps, pv, mz);
  }
  // tsl_sdf_force: -g_v of field j, the force the solid applies to the cloth, and -(x_v - c) x g_v, its torque about the field's centre
  static TSL_DEV void force(const Table& S, int j, const d3& x, const d3& xp, double (&s)[6]) {
    SphHead h;
    d3 xc;
    Sym3 Hl;
    sdf_here<1>(S, j, x, h, xc, Hl);
    if (S.row[j][SDF_MU] > 0.0) { SdfLag L; sdf_lag<1>(S, j, xp, h, L); }
    else sdf_no_lag(h);
    if (h.act || h.lam > 0.0) {
      const d3 g = sph_pair_g(h, S, x, xp);
      const d3 tq = cross(xc, g);
      s[0] = -g.x; s[1] = -g.y; s[2] = -g.z; s[3] = -tq.x; s[4] = -tq.y; s[5] = -tq.z;
    }
  }
  // tsl_sdf_grad: this reverse step's share of d(loss)/d(c_j) (3), d(loss)/d(theta_j) (3), d(loss)/d(cp_j) (3), d(loss)/d(theta_p_j) (3),
  // d(loss)/d(mu_j), d(loss)/d(r_j), each -(dg/d.)^T p_v, H_n exact; theta, theta_p: world-frame rotation vectors applied on the left
  static TSL_DEV void grad(const Table& S, int j, const d3& x, const d3& xp, const d3& pv, double (&s)[14]) {
    const double* r = S.row[j];
    SphHead h;
    d3 xc;
    Sym3 Hl;
    SdfLag L;
    sdf_here<2>(S, j, x, h, xc, Hl);
    sdf_lag<2>(S, j, xp, h, L);   // (with mu = 0 too: the column of mu)
    if (h.act || h.pen > 0.0) {
      d3 gc(0.0, 0.0, 0.0), gt(0.0, 0.0, 0.0);
      if (h.act) {
        // -(dg/dc)^T p = H_n p,  -(dg/dtheta)^T p = (x - c) x (H_n p) + p x g_n
        const d3& m = h.q;
        const double kd = S.k * (h.d - S.eps);
        gc = m * (S.k * dot(m, pv)) + sdf_RHRt(r + SDF_R, Hl, pv) * kd;
        gt = cross(xc, gc) + cross(pv, m * kd);
        s[13] = S.k * dot(m, pv);
      }
      if (h.pen > 0.0) {
        const SphFric f = sph_fric(h, x, xp, S.eh);
        const double paw = f.a * dot(f.w, pv);
        if (h.lam > 0.0) {
          // the material point R y0 rides on the pose of this step; y0 and n0 on that of the last
          const d3 Mp = sph_M(f, pv) * h.lam;
          gc = gc + Mp; gt = gt + cross(L.Ry0, Mp);
          d3 mz;
          const d3 X = sdf_prev(r, h, L, f, S.k, S.eps, pv, mz);
          const d3 gtp = cross(f.n0, mz) * h.lam - cross(L.xpc, X);
          s[6] = -X.x; s[7] = -X.y; s[8] = -X.z; s[9] = gtp.x; s[10] = gtp.y; s[11] = gtp.z;
        }
        s[12] = -((S.k * h.pen) * paw);
        if (h.d0 < S.eps) {
#pragma clang fp contract(off)   // (the product rounded on its own: it is the one sdf_prev forms, not a part of an fma here)
          s[13] -= (h.mu * S.k) * paw;
        }
      }
      s[0] = gc.x; s[1] = gc.y; s[2] = gc.z; s[3] = gt.x; s[4] = gt.y; s[5] = gt.z;
    }
  }
};
