// Host side of soft handles (tsl_set_handles, tsl_set_handles_on_faces): the checks of the two kinds of list and the gather lists of
// the handle kernels (k_handle.hpp).  Plain C++ with no device code, so that it can also be compiled into a stand-alone program (a CPU build under
// a sanitizer) without the rest of the library.  Block addresses come from Pattern::lookup (scene_tables.hpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "scene_tables.hpp"

// A vertex list.  0: the list is valid.  -1: err names the offender -- a vertex outside [0, NV), a vertex with more than one handle (the handle kernels add to a
// vertex's row without atomics: one writer per vertex), a negative or non-finite weight.  weights == nullptr: every weight is 1.
inline int handle_validate(int NV, const int32_t* verts, const double* weights, int32_t n, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n == 0) return 0;
  if (!verts) { err = "null vertex list"; return -1; }
  std::vector<unsigned char> seen((size_t)(NV > 0 ? NV : 0), 0);
  for (int32_t i = 0; i < n; i++) {
    const int v = verts[i];
    if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d out of range [0, %d)", v, NV); err = buf; return -1; }
    if (seen[v]) { snprintf(buf, sizeof(buf), "vertex %d has more than one handle", v); err = buf; return -1; }
    seen[v] = 1;
    if (weights && !(weights[i] >= 0.0 && std::isfinite(weights[i]))) {
      snprintf(buf, sizeof(buf), "weight %g of vertex %d is negative or not finite", weights[i], v); err = buf; return -1;
    }
  }
  return 0;
}

// A face list: handle i sits on face f_i = (v_0, v_1, v_2) of the scene's global face table with barycentric coordinates b_i.
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

// A handle list has nc corners per handle: 1 for a vertex list (the vertex), 3 for a face list (the vertices of the face, handle_face_corners).
// Corner a of handle i is row nc i + a of the (n x nc) corner-vertex and coordinate tables.  Entries are packed:
//   vertex list: the touched vertices ascending; under vertex vl_v[q] the entries vl_ent[vl_ptr[q] .. vl_ptr[q + 1]) = nc i + a, ascending -- handle i,
//                corner a, v_a = vl_v[q].
//   block list:  the touched blocks (v_a, v_b), diagonal ones included, ascending by (row vertex, column vertex); block q has the address bl_addr[q]
//                (Pattern::lookup) and the entries bl_ent[bl_ptr[q] .. bl_ptr[q + 1]) = nc nc i + nc a + b, ascending.
// Corners with coordinate 0 stay in the lists: the lists depend on the corners only, not on the coordinates.  With nc = 1 and one handle per vertex
// (handle_validate) both lists have one entry per handled vertex and bl_addr is the address of its diagonal block.
struct HandleLists {
  std::vector<int> vl_v, vl_ptr, vl_ent;
  std::vector<int> bl_addr, bl_ptr, bl_ent;
};

// n x 3: the vertices of the face of every handle of a valid face list (handle_face_validate)
inline std::vector<int> handle_face_corners(const int32_t* faces_tab, const int32_t* faces, int32_t n) {
  std::vector<int> cv(3 * (size_t)n);
  for (int32_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) cv[3 * (size_t)i + a] = faces_tab[3 * (size_t)faces[i] + a];
  return cv;
}

// The gather lists of a valid list with the corners cv (n x nc).  -1: err names a pair of corners of one handle without a block in the pattern, and
// the handle's face where the caller passes the face list (faces; a vertex list has none, and its diagonal blocks always exist).
inline int handle_lists(const Pattern& P, const int* cv, int32_t n, int nc, HandleLists& L, std::string& err, const int32_t* faces = nullptr) {
  char buf[256];
  L = HandleLists();
  // vertex list: (vertex, nc i + a) sorted
  std::vector<std::pair<int, int>> ve;
  ve.reserve((size_t)nc * n);
  for (int e = 0; e < nc * n; e++) ve.emplace_back(cv[e], e);
  std::sort(ve.begin(), ve.end());
  for (size_t q = 0; q < ve.size(); q++) {
    if (q == 0 || ve[q].first != ve[q - 1].first) { L.vl_v.push_back(ve[q].first); L.vl_ptr.push_back((int)q); }
    L.vl_ent.push_back(ve[q].second);
  }
  L.vl_ptr.push_back((int)ve.size());
  // block list: ((row vertex, column vertex), nc nc i + nc a + b) sorted
  std::vector<std::pair<std::pair<int, int>, int>> be;
  be.reserve((size_t)nc * nc * n);
  for (int32_t i = 0; i < n; i++)
    for (int a = 0; a < nc; a++)
      for (int b = 0; b < nc; b++) be.push_back({{cv[(size_t)nc * i + a], cv[(size_t)nc * i + b]}, nc * nc * i + nc * a + b});
  std::sort(be.begin(), be.end());
  for (size_t q = 0; q < be.size(); q++) {
    if (q == 0 || be[q].first != be[q - 1].first) {
      const int va = be[q].first.first, vb = be[q].first.second, i = be[q].second / (nc * nc);
      const int addr = P.lookup(va, vb);
      if (addr < 0) {
        if (faces) snprintf(buf, sizeof(buf), "vertices %d and %d of face %d (handle %d) have no block in the matrix pattern", va, vb, faces[i], i);
        else snprintf(buf, sizeof(buf), "vertices %d and %d of handle %d have no block in the matrix pattern", va, vb, i);
        err = buf; return -1;
      }
      L.bl_addr.push_back(addr); L.bl_ptr.push_back((int)q);
    }
    L.bl_ent.push_back(be[q].second);
  }
  L.bl_ptr.push_back((int)be.size());
  return 0;
}
