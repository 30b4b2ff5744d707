// Host side of ties (tsl_set_ties): the checks of a tie list and the slot records as they are uploaded.  Tie i binds vertex v_i to
// the point with barycentric coordinates b_i on face f_i = (t0, t1, t2) of the scene's global face table.  Plain C++ with no device code, so that it
// can also be compiled into a stand-alone program (a CPU build under a sanitizer) without the rest of the library, as handle_host.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// 0: the list is valid.  -1: err names the offender -- a face outside [0, NF), a vertex outside [0, NV), a vertex that is a corner of its own face
// (the four vertices of a constraint slot are distinct), a barycentric coordinate that is not finite or outside [0, 1], a triple whose sum differs
// from 1 by more than 1e-9, a negative or non-finite weight.  weights == nullptr: every weight is 1.  Coordinates are used as given.
inline int tie_validate(int NV, int NF, const int32_t* faces_tab, const int32_t* verts, const int32_t* faces, const double* bary, const double* weights,
                        int32_t n, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n == 0) return 0;
  if (n >= (1 << 27)) { snprintf(buf, sizeof(buf), "n = %d: too many ties for the packed row lists", n); err = buf; return -1; }
  if (!verts || !faces || !bary) { err = "null vertex list, null face list or null barycentric coordinates"; return -1; }
  for (int32_t i = 0; i < n; i++) {
    const int f = faces[i], v = verts[i];
    if (f < 0 || f >= NF || !faces_tab) { snprintf(buf, sizeof(buf), "face %d of tie %d out of range [0, %d)", f, i, NF); err = buf; return -1; }
    if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d of tie %d (face %d) out of range [0, %d)", v, i, f, NV); err = buf; return -1; }
    for (int a = 0; a < 3; a++) {
      const int t = faces_tab[3 * (size_t)f + a];
      if (t < 0 || t >= NV) { snprintf(buf, sizeof(buf), "vertex %d of face %d (tie %d) out of range [0, %d)", t, f, i, NV); err = buf; return -1; }
      if (t == v) { snprintf(buf, sizeof(buf), "vertex %d of tie %d is a corner of its own face %d", v, i, f); err = buf; return -1; }
    }
    const double* b = bary + 3 * (size_t)i;
    for (int a = 0; a < 3; a++)
      if (!(std::isfinite(b[a]) && b[a] >= 0.0 && b[a] <= 1.0)) {
        snprintf(buf, sizeof(buf), "barycentric coordinate %g of tie %d (face %d, vertex %d) is not finite or outside [0, 1]", b[a], i, f, v); err = buf; return -1;
      }
    const double sum = (b[0] + b[1]) + b[2];
    if (!(std::fabs(sum - 1.0) <= 1e-9)) {
      snprintf(buf, sizeof(buf), "barycentric coordinates (%g, %g, %g) of tie %d (face %d, vertex %d) sum to %.12g, not 1", b[0], b[1], b[2], i, f, v, sum); err = buf; return -1;
    }
    if (weights && !(weights[i] >= 0.0 && std::isfinite(weights[i]))) {
      snprintf(buf, sizeof(buf), "weight %g of tie %d (face %d, vertex %d) is negative or not finite", weights[i], i, f, v); err = buf; return -1;
    }
  }
  return 0;
}

// The records of a valid list in the layout of the constraint slots: idx (n x 4) = (t0, t1, t2, v), b (n x 3) the coordinates as given, w (n) the weights
struct TieRecords {
  std::vector<int> idx;
  std::vector<double> b, w;
};
inline TieRecords tie_records(const int32_t* faces_tab, const int32_t* verts, const int32_t* faces, const double* bary, const double* weights, int32_t n) {
  TieRecords R;
  const size_t m = (size_t)(n > 0 ? n : 0);
  R.idx.resize(4 * m); R.b.resize(3 * m); R.w.assign(m, 1.0);
  for (size_t i = 0; i < m; i++) {
    for (int a = 0; a < 3; a++) { R.idx[4 * i + a] = faces_tab[3 * (size_t)faces[i] + a]; R.b[3 * i + a] = bary[3 * i + a]; }
    R.idx[4 * i + 3] = verts[i];
    if (weights) R.w[i] = weights[i];
  }
  return R;
}

// Where the partials of the "k_tie" key of tsl_param_grad_keys lie: behind the partials of every table class (param_keys.hpp: PgLayout::total), one
// per workgroup of k_pg_tie.  The table's rows do not move when k_tie is asked with them, and k_tie's row does not depend on the other keys' rows
// beyond their total.
#define PG_TIE_KEY "k_tie"
struct PgTiePlace { size_t off, total; int cnt; };
inline PgTiePlace pg_tie_place(size_t table_total, int nb_tie) { return PgTiePlace{table_total, table_total + (size_t)(nb_tie > 0 ? nb_tie : 0), nb_tie > 0 ? nb_tie : 0}; }
