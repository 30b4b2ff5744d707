// Wind (tsl_set_wind, tsl_set_wind_velocity): lagged linear aerodynamic drag on cloth faces.  Wind face i of the list has the corners
// (v_0, v_1, v_2) of its face in the scene's face table and a weight w_i >= 0.  With x the positions and xp the start-of-step positions:
//   a   = 1/2 (xp_1 - xp_0) x (xp_2 - xp_0),  A0 = |a|                      the lagged area vector
//   M   = w_i [ c_t A0 I + (c_n - c_t) a a^T / A0 ]                         N s / m; positive semi-definite for c_n, c_t >= 0
//   r   = (xbar - xpbar) / dt - W,  xbar = (x_0 + x_1 + x_2) / 3            the centroid velocity relative to the wind
//   E_w = dt / 2 sum_i r^T M r,  gradient row of each corner: M r / 3,  block of each of the nine corner pairs: M / (9 dt).
// M depends on xp only: the blocks are constant over the Newton iterations of a step and positive semi-definite as they stand, so spd 0 / 1 / 2 and
// "spd_literal" add the same numbers.  A face with A0 < 1e-12 m^2 at the start of the step contributes nothing to any kernel.
// A face term: k_wind_face writes one record per face (structure of arrays, entry-major: entry q of face i at rec[q n + i], so that the gathers read
// a face's entry coalesced along the list), k_wind_grad adds the records of a vertex's entries (one lane per touched VERTEX) and k_wind_hess those of
// a block's entries (one lane per touched BLOCK) over the gather lists of handle_host.hpp, each in list order with one write.  No atomics, every sum
// in a fixed order: the same bits run to run.  Frozen dofs follow the rule of every other term: the assembly adds to the unmasked gradient and matrix,
// k_mask_vec / k_mask_matrix behind it take the frozen entries out again; the adjoint solution counts on its free dofs only (free_p).
// Launched only while a list exists and c_n + c_t != 0 (wind_on, wind_api.hpp).  No counterpart in the reference.
#pragma once
#include "k_shape.hpp"

#define WIND_AREA_MIN 1e-12   // m^2: below it a face has no normal and no drag

struct WindArgs {
  int n;
  const int* cv;      // n x 3  corner vertices of wind face i (original numbering)
  const double* w;    // n      weight
  double cn, ct;      // "wind_cn", "wind_ct", N s / m^3
  double dt;
  double Wx, Wy, Wz;  // the step's wind velocity
};

// The lagged geometry and the state of one wind face: a, A0 (ok: A0 >= WIND_AREA_MIN), the edges of xp, and r
struct WindFace {
  d3 a, e1, e2, r;
  double A0;
  bool ok;
};
TSL_DEV WindFace wind_face(const WindArgs& A, const double* __restrict__ pos, const double* __restrict__ prev, int i) {
  const int* __restrict__ v = A.cv + 3 * (size_t)i;
  const d3 p0 = ld3(prev, v[0]), p1 = ld3(prev, v[1]), p2 = ld3(prev, v[2]);
  WindFace f;
  f.e1 = p1 - p0; f.e2 = p2 - p0;
  f.a = cross(f.e1, f.e2) * 0.5;
  f.A0 = norm(f.a);
  f.ok = f.A0 >= WIND_AREA_MIN;
  const d3 xb = ((ld3(pos, v[0]) + ld3(pos, v[1])) + ld3(pos, v[2])) / 3.0, xpb = ((p0 + p1) + p2) / 3.0;
  f.r = (xb - xpb) / A.dt - d3(A.Wx, A.Wy, A.Wz);
  return f;
}
// M y = w [ c_t A0 y + (c_n - c_t) a (a . y) / A0 ]
TSL_DEV d3 wind_M_times(const WindArgs& A, const WindFace& f, double w, const d3& y) {
  return (y * (A.ct * f.A0) + f.a * ((A.cn - A.ct) * dot(f.a, y) / f.A0)) * w;
}

// One lane per wind face: the six entries of M's upper triangle (xx, xy, xz, yy, yz, zz) and the three of M r / 3 into rec[q n + i], q = 0 .. 8.
// A degenerate face writes zeros.  In front of k_wind_grad / k_wind_hess on their stream.
__global__ void __launch_bounds__(256) k_wind_face(WindArgs A, const double* __restrict__ pos, const double* __restrict__ prev, double* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const WindFace f = wind_face(A, pos, prev, i);
  double o[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (f.ok) {
    const double w = A.w[i], iso = w * (A.ct * f.A0), an = w * ((A.cn - A.ct) / f.A0);
    o[0] = iso + an * (f.a.x * f.a.x); o[1] = an * (f.a.x * f.a.y); o[2] = an * (f.a.x * f.a.z);
    o[3] = iso + an * (f.a.y * f.a.y); o[4] = an * (f.a.y * f.a.z); o[5] = iso + an * (f.a.z * f.a.z);
    const d3 g = wind_M_times(A, f, w, f.r) / 3.0;
    o[6] = g.x; o[7] = g.y; o[8] = g.z;
  }
#pragma unroll
  for (int q = 0; q < 9; q++) rec[(size_t)q * A.n + i] = o[q];
}

// F[v] += sum over the entries (i, a) of v of M_i r_i / 3, in list order, one addition to the row: one lane per touched vertex.  Behind k_vert_grad,
// which stores the row, in front of the gathers and k_mask_vec, on the stream of the vertex terms.
__global__ void __launch_bounds__(256) k_wind_grad(int n, HandleLists_dev L, const double* __restrict__ rec, double* __restrict__ F) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_vert) return;
  const int v = L.vl_v[q];
  d3 s(0.0, 0.0, 0.0);
  for (int e = L.vl_ptr[q], e1 = L.vl_ptr[q + 1]; e < e1; e++) {
    const int i = L.vl_ent[e] / 3;
    s = s + d3(rec[(size_t)6 * n + i], rec[(size_t)7 * n + i], rec[(size_t)8 * n + i]);
  }
  st3(F, v, ld3(F, v) + s);
}

// block (v_a, v_b) += sum over the block's entries (i, a, b) of M_i / (9 dt), in list order: one lane per touched block.  The upper triangle and its
// mirror are written from the same six sums (Sym3::stamp), and blocks (v_a, v_b) and (v_b, v_a) hold the same faces in the same order: the wind part
// of the matrix is symmetric bit for bit.  Behind k_vert_hess (one writer at a time per block, all on one stream), in front of the gathers and
// k_mask_matrix.
__global__ void __launch_bounds__(256) k_wind_hess(int n, double nine_dt, HandleLists_dev L, const double* __restrict__ rec, double* __restrict__ vals) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_blk) return;
  Sym3 H;
  for (int e = L.bl_ptr[q], e1 = L.bl_ptr[q + 1]; e < e1; e++) {
    const int i = L.bl_ent[e] / 9;
    H.xx += rec[i] / nine_dt; H.xy += rec[(size_t)n + i] / nine_dt; H.xz += rec[(size_t)2 * n + i] / nine_dt;
    H.yy += rec[(size_t)3 * n + i] / nine_dt; H.yz += rec[(size_t)4 * n + i] / nine_dt; H.zz += rec[(size_t)5 * n + i] / nine_dt;
  }
  H.stamp(vals, (size_t)L.bl_addr[q]);
}

// one partial per workgroup (wg_join); k_energy_final adds the partials (behind the colliders') in its fixed order
__global__ void __launch_bounds__(256) k_wind_energy(WindArgs A, const double* __restrict__ pos, const double* __restrict__ prev, double* __restrict__ e_part) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  if (i < A.n) {
    const WindFace f = wind_face(A, pos, prev, i);
    if (f.ok) e[0] = 0.5 * A.dt * dot(f.r, wind_M_times(A, f, A.w[i], f.r));
  }
  wg_join<1>(e, e_part + blockIdx.x);
}

// The reverse step, first half: pos = x_s, prev = x_{s-1}, p the adjoint solution (its frozen dofs do not count).  One lane per wind face writes
// -(dg / dx_prev)^T p of its three corners into stage[3 (3 i + a) .. + 3), with P = p_0 + p_1 + p_2 on free dofs:
//   through r:  M P / (9 dt) to each corner
//   through a:  q = 1/3 w [ c_t (P.r) a / A0 + (c_n - c_t) ( ((a.r) P + (a.P) r) / A0 - (a.P)(a.r) a / A0^3 ) ],
//               corner 1: -1/2 (e2 x q),  corner 2: -1/2 (q x e1),  corner 0: minus the sum of those two.
// A degenerate face writes zeros.
__global__ void __launch_bounds__(256) k_wind_backprop_face(WindArgs A, const int* __restrict__ frozen, const double* __restrict__ pos, const double* __restrict__ prev,
                                                            const double* __restrict__ p, double* __restrict__ stage) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const WindFace f = wind_face(A, pos, prev, i);
  d3 c0(0.0, 0.0, 0.0), c1(0.0, 0.0, 0.0), c2(0.0, 0.0, 0.0);
  if (f.ok) {
    const int* __restrict__ v = A.cv + 3 * (size_t)i;
    const double w = A.w[i];
    const d3 P = (free_p(frozen, p, v[0]) + free_p(frozen, p, v[1])) + free_p(frozen, p, v[2]);
    const d3 thr = wind_M_times(A, f, w, P) / (9.0 * A.dt);
    const double Pr = dot(P, f.r), ar = dot(f.a, f.r), aP = dot(f.a, P);
    const d3 q = (f.a * (A.ct * Pr / f.A0) + ((P * ar + f.r * aP) / f.A0 - f.a * (aP * ar / (f.A0 * f.A0 * f.A0))) * (A.cn - A.ct)) * (w / 3.0);
    const d3 t1 = cross(f.e2, q) * -0.5, t2 = cross(q, f.e1) * -0.5;
    c1 = thr + t1; c2 = thr + t2; c0 = thr - (t1 + t2);
  }
  st3(stage, 3 * i, c0); st3(stage, 3 * i + 1, c1); st3(stage, 3 * i + 2, c2);
}
// second half: one lane per touched vertex adds the staged values of its entries in list order to its row of pos_grad[s-1], on free dofs
// (add_free).  In front of k_adj_prev.
__global__ void __launch_bounds__(256) k_wind_backprop(HandleLists_dev L, const int* __restrict__ frozen, const double* __restrict__ stage, double* __restrict__ pg_prev) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L.n_vert) return;
  d3 s(0.0, 0.0, 0.0);
  for (int e = L.vl_ptr[q], e1 = L.vl_ptr[q + 1]; e < e1; e++) s = s + ld3(stage, L.vl_ent[e]);
  add_free(frozen, pg_prev, L.vl_v[q], s);
}

// Read-outs: one lane per wind face, N sums joined per workgroup (wg_join<N>) into part[N blockIdx.x ..]; k_wind_join adds the workgroups in index order.
//   N = 3 (tsl_wind_force): -sum_i M_i r_i, the net force the wind applies to the cloth; frozen dofs are not masked; p and frozen are not read
//   N = 5 (tsl_wind_grad):  this reverse step's share of d(loss)/d(W, c_n, c_t), each -sum (dg/d.)^T p on the free dofs of p:
//     [0:3] +1/3 sum_i M_i P_i,  [3] -1/3 sum_i w_i A0 (n0.r)(n0.P),  [4] -1/3 sum_i w_i A0 (r.P - (n0.r)(n0.P))
template <int N>
__global__ void __launch_bounds__(256) k_wind_readout(WindArgs A, const int* __restrict__ frozen, const double* __restrict__ pos, const double* __restrict__ prev,
                                                      const double* __restrict__ p, double* __restrict__ part) {
  static_assert(N == 3 || N == 5, "k_wind_readout: 3 (force) or 5 (gradient) values");
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double s[N];
#pragma unroll
  for (int q = 0; q < N; q++) s[q] = 0.0;
  if (i < A.n) {
    const WindFace f = wind_face(A, pos, prev, i);
    if (f.ok) {
      const double w = A.w[i];
      if constexpr (N == 3) {
        const d3 g = wind_M_times(A, f, w, f.r);
        s[0] = -g.x; s[1] = -g.y; s[2] = -g.z;
      } else {
        const int* __restrict__ v = A.cv + 3 * (size_t)i;
        const d3 P = (free_p(frozen, p, v[0]) + free_p(frozen, p, v[1])) + free_p(frozen, p, v[2]);
        const d3 MP = wind_M_times(A, f, w, P) / 3.0;
        const double nn = dot(f.a, f.r) * dot(f.a, P) / (f.A0 * f.A0);   // (n0.r)(n0.P)
        s[0] = MP.x; s[1] = MP.y; s[2] = MP.z;
        s[3] = -(w * f.A0) * nn / 3.0;
        s[4] = -(w * f.A0) * (dot(f.r, P) - nn) / 3.0;
      }
    }
  }
  wg_join<N>(s, part + (size_t)N * blockIdx.x);
}
// out[q] = part[0][q] + part[1][q] + ..., in workgroup order: one lane per value
__global__ void k_wind_join(int n_wg, int N, const double* __restrict__ part, double* __restrict__ out) {
  const int q = threadIdx.x;
  if (q >= N) return;
  double t = 0.0;
  for (int w = 0; w < n_wg; w++) t += part[(size_t)N * w + q];
  out[q] = t;
}
