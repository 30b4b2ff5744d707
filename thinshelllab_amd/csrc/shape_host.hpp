// Host side that the five collider kinds share: the table a kind's kernels take, the per-vertex mask and the checks that differ
// between the kinds only in a noun ("collider", "sphere", "capsule", "box", "field").  What is particular to a kind -- its rows and their checks -- is in
// collider_host.hpp, sphere_host.hpp, capsule_host.hpp, box_host.hpp and sdf_host.hpp.  Plain C++ with no device code, so that it can also be compiled into a stand-alone
// program (a CPU build under a sanitizer) without the rest of the library, as tie_host.hpp.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// shapes of one kind: bit j of a vertex's mask byte stands for shape j
#define SHAPE_MAX 8
static_assert(SHAPE_MAX == CHAR_BIT * sizeof(uint8_t), "the mask is one byte per vertex, one bit per shape");

// The table of one kind, passed to every kernel of the kind BY VALUE (no global array): n shapes, row j the W doubles of shape j as the kind's
// header lays them out.  k: the kind's stiffness, eps: the scene's eps_contact (thickness of the shell), eh: eps_v dt (the friction
// regularisation of fr_f0 / fr_f1 / fr_f2); the three are filled in per launch
template <int W>
struct ShapeTable {
  static constexpr int width = W;
  int n;
  double k, eps, eh;
  double row[SHAPE_MAX][W];
};

static inline bool finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

// The checks of a list's length, and Q := T with n shapes and every row zero.  0, or -1 with err set: n < 0, n > SHAPE_MAX, or has_null (a null
// array where n > 0), whose message is null_msg
template <int W>
inline int shape_count_check(const char* noun, int32_t n, bool has_null, const char* null_msg, const ShapeTable<W>& T, ShapeTable<W>& Q, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n > SHAPE_MAX) { snprintf(buf, sizeof(buf), "%d %ss: at most %d", n, noun, SHAPE_MAX); err = buf; return -1; }
  if (n > 0 && has_null) { err = null_msg; return -1; }
  Q = T;
  Q.n = n;
  for (int32_t j = 0; j < SHAPE_MAX; j++)
    for (int q = 0; q < W; q++) Q.row[j][q] = 0.0;
  return 0;
}
inline int shape_radius_check(const char* noun, double R, int j, std::string& err) {
  char buf[256];
  if (std::isfinite(R) && R > 0.0) return 0;
  snprintf(buf, sizeof(buf), "radius %g of %s %d is not finite and positive", R, noun, j); err = buf; return -1;
}
inline int shape_mu_check(const char* noun, double mu, int j, std::string& err) {
  char buf[256];
  if (mu >= 0.0 && std::isfinite(mu)) return 0;
  snprintf(buf, sizeof(buf), "friction coefficient %g of %s %d is negative or not finite", mu, noun, j); err = buf; return -1;
}

// The per-vertex mask (NV bytes, bit j: shape j acts on the vertex).  mask == nullptr: every one of the n shapes on every vertex.  -1, naming
// the vertex, for a byte with a bit at or above n (out untouched)
inline int shape_mask_validate(const char* noun, int NV, int32_t n, const uint8_t* mask, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  const unsigned all = n >= 8 ? 0xffu : ((1u << (n > 0 ? n : 0)) - 1u);
  if (!mask) { out.assign((size_t)NV, (uint8_t)all); return 0; }
  for (int v = 0; v < NV; v++)
    if (mask[v] & ~all) { snprintf(buf, sizeof(buf), "mask 0x%02x of vertex %d names a %s at or above %d", (unsigned)mask[v], v, noun, n); err = buf; return -1; }
  out.assign(mask, mask + NV);
  return 0;
}

// The mask from vertex lists, for callers that hold ids: the ids of shape j are ids[ptr[j] .. ptr[j + 1]).  -1, naming shape and vertex, for an
// id outside [0, NV) (out untouched)
inline int shape_mask_from_ids(const char* noun, int NV, int32_t n, const int32_t* ptr, const int32_t* ids, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  std::vector<uint8_t> m((size_t)NV, 0);
  for (int32_t j = 0; j < n && j < SHAPE_MAX; j++)
    for (int32_t e = ptr[j]; e < ptr[j + 1]; e++) {
      const int v = ids[e];
      if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d of %s %d out of range [0, %d)", v, noun, j, NV); err = buf; return -1; }
      m[(size_t)v] |= (uint8_t)(1u << j);
    }
  out.swap(m);
  return 0;
}
