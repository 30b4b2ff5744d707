// Host side of soft handles at barycentric points of faces (tsl_set_handles_on_faces): the checks of the list and the two gather
// lists of the face-handle kernels (k_handle_face.hpp).  Plain C++ with no device code, so that it can also be compiled into a stand-alone
// program (a CPU build under a sanitizer) without the rest of the library.  Block addresses come from Pattern::lookup (scene_tables.hpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "scene_tables.hpp"

// Handle i sits on face f_i = (v_0, v_1, v_2) of the scene's global face table with barycentric coordinates b_i.  Entries are packed:
//   vertex list: the touched vertices ascending; under vertex vl_v[q] the entries vl_ent[vl_ptr[q] .. vl_ptr[q + 1]) = 3 i + a, ascending -- handle i,
//                corner a, v_a = vl_v[q]; 3 i + a is also the row of the corner in the (n x 3) vertex and coordinate tables.
//   block list:  the touched blocks (v_a, v_b), diagonal ones included, ascending by (row vertex, column vertex); block q has the address bl_addr[q]
//                (Pattern::lookup) and the entries bl_ent[bl_ptr[q] .. bl_ptr[q + 1]) = 9 i + 3 a + b, ascending.
// Corners with b_a = 0 stay in the lists: the lists depend on the faces only, not on the coordinates.
struct FaceHandleLists {
  std::vector<int> fv;                       // n x 3  vertices of the face of handle i
  std::vector<int> vl_v, vl_ptr, vl_ent;
  std::vector<int> bl_addr, bl_ptr, bl_ent;
};

// 0: the list is valid.  -1: err names the offender -- a face outside [0, NF), a barycentric coordinate that is not finite or outside [0, 1], a triple
// whose sum differs from 1 by more than 1e-9, a negative or non-finite weight, a vertex of the face outside [0, NV).  weights == nullptr: every weight is 1.
inline int handle_face_validate(int NV, int NF, const int32_t* faces_tab, const int32_t* faces, const double* bary, const double* weights, int32_t n,
                                std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n == 0) return 0;
  if (n >= (1 << 27)) { snprintf(buf, sizeof(buf), "n = %d: too many handles for the packed gather lists", n); err = buf; return -1; }
  if (!faces || !bary) { err = "null face list or null barycentric coordinates"; return -1; }
  for (int32_t i = 0; i < n; i++) {
    const int f = faces[i];
    if (f < 0 || f >= NF || !faces_tab) { snprintf(buf, sizeof(buf), "face %d of handle %d out of range [0, %d)", f, i, NF); err = buf; return -1; }
    const double* b = bary + 3 * (size_t)i;
    for (int a = 0; a < 3; a++)
      if (!(std::isfinite(b[a]) && b[a] >= 0.0 && b[a] <= 1.0)) {
        snprintf(buf, sizeof(buf), "barycentric coordinate %g of handle %d (face %d) is not finite or outside [0, 1]", b[a], i, f); err = buf; return -1;
      }
    const double sum = (b[0] + b[1]) + b[2];
    if (!(std::fabs(sum - 1.0) <= 1e-9)) {
      snprintf(buf, sizeof(buf), "barycentric coordinates (%g, %g, %g) of handle %d (face %d) sum to %.12g, not 1", b[0], b[1], b[2], i, f, sum); err = buf; return -1;
    }
    if (weights && !(weights[i] >= 0.0 && std::isfinite(weights[i]))) {
      snprintf(buf, sizeof(buf), "weight %g of handle %d (face %d) is negative or not finite", weights[i], i, f); err = buf; return -1;
    }
    for (int a = 0; a < 3; a++) {
      const int v = faces_tab[3 * (size_t)f + a];
      if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d of face %d (handle %d) out of range [0, %d)", v, f, i, NV); err = buf; return -1; }
    }
  }
  return 0;
}

// The gather lists of a valid list (handle_face_validate).  -1: err names a pair of the face's vertices without a block in the pattern.
inline int handle_face_lists(const Pattern& P, const int32_t* faces_tab, const int32_t* faces, int32_t n, FaceHandleLists& L, std::string& err) {
  char buf[256];
  L = FaceHandleLists();
  L.fv.resize(3 * (size_t)n);
  for (int32_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) L.fv[3 * (size_t)i + a] = faces_tab[3 * (size_t)faces[i] + a];
  // vertex list: (vertex, 3 i + a) sorted
  std::vector<std::pair<int, int>> ve;
  ve.reserve(3 * (size_t)n);
  for (int e = 0; e < 3 * n; e++) ve.emplace_back(L.fv[e], e);
  std::sort(ve.begin(), ve.end());
  for (size_t q = 0; q < ve.size(); q++) {
    if (q == 0 || ve[q].first != ve[q - 1].first) { L.vl_v.push_back(ve[q].first); L.vl_ptr.push_back((int)q); }
    L.vl_ent.push_back(ve[q].second);
  }
  L.vl_ptr.push_back((int)ve.size());
  // block list: ((row vertex, column vertex), 9 i + 3 a + b) sorted
  std::vector<std::pair<std::pair<int, int>, int>> be;
  be.reserve(9 * (size_t)n);
  for (int32_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) be.push_back({{L.fv[3 * (size_t)i + a], L.fv[3 * (size_t)i + b]}, 9 * i + 3 * a + b});
  std::sort(be.begin(), be.end());
  for (size_t q = 0; q < be.size(); q++) {
    if (q == 0 || be[q].first != be[q - 1].first) {
      const int va = be[q].first.first, vb = be[q].first.second;
      const int addr = P.lookup(va, vb);
      if (addr < 0) {
        snprintf(buf, sizeof(buf), "vertices %d and %d of face %d (handle %d) have no block in the matrix pattern", va, vb, faces[be[q].second / 9], be[q].second / 9);
        err = buf; return -1;
      }
      L.bl_addr.push_back(addr); L.bl_ptr.push_back((int)q);
    }
    L.bl_ent.push_back(be[q].second);
  }
  L.bl_ptr.push_back((int)be.size());
  return 0;
}
