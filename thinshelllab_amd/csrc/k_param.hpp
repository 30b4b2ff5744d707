// Parameter vector-Jacobian products of the system-identification adjoint (tsl_param_grad_keys): for every material or contact scalar theta,
// -sum over the free dofs of p . dF/d(theta), F the gradient tsl_assemble forms (so the value is p . d(force)/d(theta), the sign of tsl_param_grad).
// Every supported scalar enters F linearly, so an element's dF/d(theta) is its own gradient term with the scalar set to one; the terms below
// restate the forward kernels' expressions (k_cloth_grad_face, k_cloth_grad_hinge, k_tet_grad, k_contact_assemble_coop, k_handle_grad) through the same device
// functions (load_face, face_geom, hinge_grad, dihedral, tet_F, m3_cof2, fr_f1) without touching those kernels.
// One pass per element class, one lane per element, no per-vertex gather: the element dots its dF/d(theta) with p at its free dofs, the workgroup
// joins the lanes by the fixed tree of block_sum and writes ONE partial per key (part[key_row * gridDim.x + blockIdx.x]); k_pg_final sums a key's
// partials in a fixed order.  No atomics: a key's value is the same bits whichever other keys a call asks for.
#pragma once
#include "k_cloth.hpp"
#include "k_contact.hpp"
#include "k_fem.hpp"
#include "k_handle.hpp"
#include "param_keys.hpp"
#include "tsl_device.hpp"

#define PG_THREADS 256

// p . g over the free dofs of vertex v
TSL_DEV double pg_dot_free(const double* __restrict__ p, const int* __restrict__ frozen, int v, const d3& g) {
  double s = 0.0;
  if (!frozen[3 * v]) s += p[3 * v] * g.x;
  if (!frozen[3 * v + 1]) s += p[3 * v + 1] * g.y;
  if (!frozen[3 * v + 2]) s += p[3 * v + 2] * g.z;
  return s;
}

// Workgroup partials of NK keys per group (cloth, body): the lane's values v[] count for group g (-1: none).  Row (q NK + k) of part holds
// the partials of key k of group q.  Every thread of the workgroup takes part (block_sum synchronises); a group no lane of the workgroup
// belongs to gets a zero partial without a reduction.
template <int NK>
TSL_DEV void pg_block_write(const double v[NK], int g, int n_group, double* __restrict__ part, double* sm) {
  for (int q = 0; q < n_group; q++) {
    const bool any = __syncthreads_or(g == q);
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const double r = any ? block_sum(g == q ? v[k] : 0.0, sm) : 0.0;
      if (threadIdx.x == 0) part[(size_t)(q * NK + k) * gridDim.x + blockIdx.x] = r;
    }
  }
}

// faces: {Kl, Ka} of cloth cid[f] -- the spring and area terms of k_cloth_grad_face with Kl = Ka = 1.  STVK (some cloth has membrane = 1): the faces
// of such cloths have no spring or area term and add exact zeros
template <bool STVK = false>
__global__ void __launch_bounds__(PG_THREADS) k_pg_face(ClothArgs A, int n_cloth, const double* __restrict__ pos, const double* __restrict__ p,
                                                        const int* __restrict__ frozen, double* __restrict__ part, StvkArgs S) {
  __shared__ double sm[PG_THREADS / 64];
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  double v[2] = {0.0, 0.0};
  int g = -1;
  if (f < A.n_cface) {
    g = A.cid[f];
    if (!STVK || S.stvk[4 * g] == 0.0) {
      int vi[3]; d3 P[3];
      load_face(pos, A.f2v, f, vi, P);
      d3 gl[3] = {d3(), d3(), d3()};
#pragma unroll
      for (int l = 0; l < 3; l++) {
        const int m = (l + 1) % 3;
        const d3 delta = P[l] - P[m];
        const double len = norm(delta);
        const d3 t = delta * (-2.0 * (1.0 - len / A.li[3 * f + l]) / len);
        gl[l] = gl[l] + t;
        gl[m] = gl[m] - t;
      }
      const d3 Nn = cross(P[1] - P[0], P[2] - P[0]);
      const double nN = norm(Nn);
      const double da = -2.0 * (1.0 - 0.5 * nN / A.V[f]);
      const d3 nh = Nn / nN;
#pragma unroll
      for (int l = 0; l < 3; l++) {
        v[0] -= pg_dot_free(p, frozen, vi[l], gl[l]);
        v[1] -= pg_dot_free(p, frozen, vi[l], da * (0.5 * cross(nh, P[(l + 2) % 3] - P[(l + 1) % 3])));
      }
    }
  }
  pg_block_write<2>(v, g, n_cloth, part, sm);
}

// faces: {stvk_mu, stvk_lam} of cloth cid[f] -- the StVK gradient of k_cloth_grad_face<true> with (mu, lam) = (1, 0) and (0, 1); faces of cloths
// with membrane = 0 add exact zeros
__global__ void __launch_bounds__(PG_THREADS) k_pg_stvk(ClothArgs A, int n_cloth, const double* __restrict__ pos, const double* __restrict__ p,
                                                        const int* __restrict__ frozen, double* __restrict__ part, StvkArgs S) {
  __shared__ double sm[PG_THREADS / 64];
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  double v[2] = {0.0, 0.0};
  int g = -1;
  if (f < A.n_cface) {
    g = A.cid[f];
    if (S.stvk[4 * g] != 0.0) {
      int vi[3]; d3 P[3];
      load_face(pos, A.f2v, f, vi, P);
      const StvkFace s = stvk_face(P, S.dminv + 4 * f);
      d3 gm[3], gl[3];
      stvk_grad(s, 1.0, 0.0, A.V[f], gm);
      stvk_grad(s, 0.0, 1.0, A.V[f], gl);
#pragma unroll
      for (int l = 0; l < 3; l++) {
        v[0] -= pg_dot_free(p, frozen, vi[l], gm[l]);
        v[1] -= pg_dot_free(p, frozen, vi[l], gl[l]);
      }
    }
  }
  pg_block_write<2>(v, g, n_cloth, part, sm);
}

// hinges: {Kb} of cloth cid[f1] -- k_cloth_grad_hinge with Kb = 1; the four gradients belong to hg_v[4 h + j]
__global__ void __launch_bounds__(PG_THREADS) k_pg_hinge(ClothArgs A, int n_cloth, const double* __restrict__ pos, const double* __restrict__ ref_angle,
                                                         const double* __restrict__ p, const int* __restrict__ frozen, double* __restrict__ part) {
  __shared__ double sm[PG_THREADS / 64];
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  double v[1] = {0.0};
  int g = -1;
  if (h < A.n_hinge) {
    const int f1 = A.hg_info[8 * h], l = A.hg_info[8 * h + 1], f2 = A.hg_info[8 * h + 2], p4 = A.hg_info[8 * h + 3], p21 = A.hg_info[8 * h + 4];
    g = A.cid[f1];
    const ClothDev c = A.cloth[g];
    int v1[3], v2[3]; d3 P1[3], P2[3];
    load_face(pos, A.f2v, f1, v1, P1);
    load_face(pos, A.f2v, f2, v2, P2);
    const FaceGeom g1 = face_geom(P1), g2 = face_geom(P2);
    d3 gr[4];
    hinge_grad(g1, g2, l, p4, p21, gr);
    const double theta = dihedral(g1.n, g2.n, pick3(P1, (l + 1) % 2) - pick3(P1, l));
    const double dth = 2.0 * (theta - ref_angle[3 * f1 + l]) * c.dx * c.dx * (1.0 / 3.0);
#pragma unroll
    for (int j = 0; j < 4; j++) v[0] -= pg_dot_free(p, frozen, A.hg_v[4 * h + j], dth * gr[j]);
  }
  pg_block_write<1>(v, g, n_cloth, part, sm);
}

// tetrahedra: {mu, lam} of body tel[t] -- dP/d(mu), dP/d(lam) of k_tet_grad for both material models (alpha fixed)
__global__ void __launch_bounds__(PG_THREADS) k_pg_tet(TetArgs A, int n_el, const double* __restrict__ pos, const double* __restrict__ p,
                                                       const int* __restrict__ frozen, double* __restrict__ part) {
  __shared__ double sm[PG_THREADS / 64];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  double v[2] = {0.0, 0.0};
  int g = -1;
  if (t < A.n_tet) {
    int vi[4]; m3 B;
    const m3 F = tet_F(A, t, pos, vi, B);
    g = A.tel[t];
    const ElasticDev e = A.el[g];
    m3 Pm, Pl;
    if (e.kind == 0) {   // P = mu F + lam (J - alpha) cof(F)
      const double J = m3_det(F);
      const m3 C = m3_cof2(F, F);
#pragma unroll
      for (int k = 0; k < 9; k++) { Pm.m[k] = F.m[k]; Pl.m[k] = (J - e.alpha) * C.m[k]; }
    } else {             // P = mu (F - F^-T) + lam log(max(J, 0.01)) F^-T
      const m3 FiT = m3_T(m3_inv(F));
      const double lj = log(fmax(m3_det(F), 0.01));
#pragma unroll
      for (int k = 0; k < 9; k++) { Pm.m[k] = F.m[k] - FiT.m[k]; Pl.m[k] = lj * FiT.m[k]; }
    }
    const m3 BT = m3_T(B);
    const m3 Hm = m3_mul(Pm, BT), Hl = m3_mul(Pl, BT);
    const double W = A.W[t];
    d3 sm3 = d3(), sl3 = d3();
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const d3 gm = d3(W * Hm.m[i], W * Hm.m[3 + i], W * Hm.m[6 + i]), gl = d3(W * Hl.m[i], W * Hl.m[3 + i], W * Hl.m[6 + i]);
      v[0] -= pg_dot_free(p, frozen, vi[i], gm);
      v[1] -= pg_dot_free(p, frozen, vi[i], gl);
      sm3 = sm3 - gm; sl3 = sl3 - gl;
    }
    v[0] -= pg_dot_free(p, frozen, vi[3], sm3);
    v[1] -= pg_dot_free(p, frozen, vi[3], sl3);
  }
  pg_block_write<2>(v, g, n_el, part, sm);
}

// vertex-triangle contact slots: {k_contact, mu_cloth_elastic, mu_cloth_cloth}.  Normal term of k_contact_assemble_coop: grad d (d - eps) on the
// active slots; friction term with the lagged weight c_k = -mu k_contact (gap - eps) of the detection, whose derivative is c_k / k_contact and,
// on the slots of a live friction parameter (c_kind 1 / 2), c_k / mu_live (the pair's factor, e.g. Scene_card's x10, stays inside c_k).
__global__ void __launch_bounds__(PG_THREADS) k_pg_contact(int nc, ContactArgs A, const int* __restrict__ kind, double mu_ce, double mu_cc,
                                                           const double* __restrict__ pos, const double* __restrict__ p, const int* __restrict__ frozen,
                                                           double* __restrict__ part) {
  __shared__ double sm[PG_THREADS / 64];
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (ci < nc) {
    int id[4];
    for (int k = 0; k < 4; k++) id[k] = A.idx[4 * ci + k];
    const d3 x0 = ld3(pos, id[0]), xa = ld3(pos, id[1]), xb = ld3(pos, id[2]), xp = ld3(pos, id[3]);
    // normal: d = D / C, D = p . (a x b), C = |a x b| in q = (a, b, p) = (xa - x0, xb - x0, xp - x0); vertex 0 takes minus the sum
    const d3 a = xa - x0, b = xb - x0, q = xp - x0;
    const d3 cr = cross(a, b);
    const double D = dot(cr, q), C = norm(cr);
    double sn = 0.0;
    if (D / C < A.eps_contact) {
      const d3 nh = cr / C;
      const double s = D / C - A.eps_contact, iC = 1.0 / C, DC2 = D / (C * C);
      const d3 G1 = (cross(b, q) * iC - cross(b, nh) * DC2) * s, G2 = (cross(q, a) * iC - cross(nh, a) * DC2) * s, G3 = cr * (iC * s);
      sn = pg_dot_free(p, frozen, id[1], G1) + pg_dot_free(p, frozen, id[2], G2) + pg_dot_free(p, frozen, id[3], G3) -
           pg_dot_free(p, frozen, id[0], G1 + G2 + G3);
    }
    // friction per unit c_k: w1_i f1(r) T^T u at vertex i, w1 = (-w0, -w1, -w2, 1)
    const double w[3] = {A.w[3 * ci], A.w[3 * ci + 1], A.w[3 * ci + 2]};
    const double* T = A.T + 6 * (size_t)ci;
    const d3 dx = xp - (x0 * w[0] + xa * w[1] + xb * w[2]) - ld3(A.dx0, ci);
    const double u0 = T[0] * dx.x + T[1] * dx.y + T[2] * dx.z, u1 = T[3] * dx.x + T[4] * dx.y + T[5] * dx.z;
    const double f1 = fr_f1(sqrt(u0 * u0 + u1 * u1), A.eps_vh);
    const d3 tu = d3(u0 * T[0] + u1 * T[3], u0 * T[1] + u1 * T[4], u0 * T[2] + u1 * T[5]) * f1;
    const double sf = pg_dot_free(p, frozen, id[3], tu) - w[0] * pg_dot_free(p, frozen, id[0], tu) - w[1] * pg_dot_free(p, frozen, id[1], tu) -
                      w[2] * pg_dot_free(p, frozen, id[2], tu);
    const double kf = A.k[ci];
    const int kd = kind[ci];
    v[0] = -(sn + sf * (kf / A.k_contact));
    if (kd == 1) v[1] = -sf * (kf / mu_ce);
    if (kd == 2) v[2] = -sf * (kf / mu_cc);
  }
  pg_block_write<3>(v, ci < nc ? 0 : -1, 1, part, sm);
}

// One workgroup: out[j] = sum of the partials [off[j], off[j] + cnt[j]) of key j, lanes strided, joined by block_sum (a fixed tree per key).  The
// table travels as a kernel argument (no upload); a call with more than PG_KEYS_PER_LAUNCH keys launches this kernel once per chunk of keys, out
// pointing at the chunk (PgTable: param_keys.hpp).  With n_ee > 0 it also counts the edge-edge slots kinds[0 .. n_ee) of kind 1 and 2 into
// cnt_out[0], cnt_out[1].
__global__ void __launch_bounds__(PG_THREADS) k_pg_final(PgTable tab, const double* __restrict__ part, int n_ee, const int* __restrict__ kinds,
                                                         double* __restrict__ out, double* __restrict__ cnt_out) {
  __shared__ double sm[PG_THREADS / 64];
  for (int j = 0; j < tab.n; j++) {
    const int o = tab.off[j], n = tab.cnt[j];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += part[(size_t)o + i];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) out[j] = s;
  }
  if (!cnt_out) return;
  double k1 = 0.0, k2 = 0.0;
  for (int i = threadIdx.x; i < n_ee; i += blockDim.x) { k1 += kinds[i] == 1 ? 1.0 : 0.0; k2 += kinds[i] == 2 ? 1.0 : 0.0; }
  k1 = block_sum(k1, sm);
  k2 = block_sum(k2, sm);
  if (threadIdx.x == 0) { cnt_out[0] = k1; cnt_out[1] = k2; }
}

// soft handles: {k_handle} -- the gradient rows of k_handle_grad with k_handle = 1, w_i b_a (p_i - t_i) at the corners v_a of handle i (class 5):
// -w_i sum_a b_a p_{v_a} . (p_i - t_i) over free dofs; one lane per handle
template <int NC>
__global__ void __launch_bounds__(PG_THREADS) k_pg_handle(HandleArgs A, const double* __restrict__ pos, const double* __restrict__ p,
                                                          const int* __restrict__ frozen, double* __restrict__ part) {
  __shared__ double sm[PG_THREADS / 64];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double v[1] = {0.0};
  if (i < A.n) {
    const d3 r = handle_point<NC>(A, pos, i) - ld3(A.t, i);
    if constexpr (NC == 1) {
      v[0] = -pg_dot_free(p, frozen, A.cv[i], r * A.w[i]);
    } else {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 3; a++) s += pg_dot_free(p, frozen, A.cv[3 * (size_t)i + a], r * (A.w[i] * A.cb[3 * (size_t)i + a]));
      v[0] = -s;
    }
  }
  pg_block_write<1>(v, i < A.n ? 0 : -1, 1, part, sm);
}
