// Host side of the half-space colliders (tsl_set_colliders): the checks of a collider list and the plane table as the kernels take
// it.  Collider j is the half-space n_j . x < o_j (the solid side) with a unit normal n_j, fixed once the list is set, an offset o_j that may be
// set before every step, and a friction coefficient mu_j >= 0.  Plain C++ with no device code, so that it can also be compiled into a stand-alone
// program (a CPU build under a sanitizer) without the rest of the library, as tie_host.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifndef TSL_MAX_COLLIDERS
#define TSL_MAX_COLLIDERS 8
#endif

// The plane table, passed to every collider kernel BY VALUE (no global array): row j = (n (3), o, mu, t1 (3), t2 (3)), 11 doubles.  k: "k_collider",
// eps: the scene's eps_contact (thickness of the shell), eh: eps_v dt (the friction regularisation of fr_f0 / fr_f1 / fr_f2)
struct ColliderPlanes {
  int n;
  double k, eps, eh;
  double pl[TSL_MAX_COLLIDERS][11];
};

// 0: the list is valid and P holds it (normals normalised, the tangent pair T = (t1, t2) built from the unit normal exactly as k_contact_pair builds
// c_T; k, eps, eh are left alone).  -1: err names the offender and P is untouched -- more than TSL_MAX_COLLIDERS colliders, a normal that is
// zero or not finite, an offset that is not finite, a friction coefficient that is negative or not finite.
inline int collider_validate(const double* normals, const double* offsets, const double* mu, int32_t n, ColliderPlanes& P, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n > TSL_MAX_COLLIDERS) { snprintf(buf, sizeof(buf), "%d colliders: at most %d", n, TSL_MAX_COLLIDERS); err = buf; return -1; }
  if (n > 0 && (!normals || !offsets || !mu)) { err = "null normals, null offsets or null friction coefficients"; return -1; }
  ColliderPlanes Q = P;
  Q.n = n;
  for (int32_t j = 0; j < TSL_MAX_COLLIDERS; j++)
    for (int q = 0; q < 11; q++) Q.pl[j][q] = 0.0;
  for (int32_t j = 0; j < n; j++) {
    const double* a = normals + 3 * (size_t)j;
    const double len = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if (!(std::isfinite(len) && len > 0.0)) {
      snprintf(buf, sizeof(buf), "normal (%g, %g, %g) of collider %d is zero or not finite", a[0], a[1], a[2], j); err = buf; return -1;
    }
    if (!std::isfinite(offsets[j])) { snprintf(buf, sizeof(buf), "offset %g of collider %d is not finite", offsets[j], j); err = buf; return -1; }
    if (!(mu[j] >= 0.0 && std::isfinite(mu[j]))) { snprintf(buf, sizeof(buf), "friction coefficient %g of collider %d is negative or not finite", mu[j], j); err = buf; return -1; }
    const double nx = a[0] / len, ny = a[1] / len, nz = a[2] / len;
    // t1 = |n.x| < 0.5 ? (n.x, n.z, -n.y) : (n.y, -n.x, n.z);  t2 = n x t1;  t1 = n x t2   (k_contact_pair)
    double t1[3], t2[3];
    if (std::fabs(nx) < 0.5) { t1[0] = nx; t1[1] = nz; t1[2] = -ny; } else { t1[0] = ny; t1[1] = -nx; t1[2] = nz; }
    t2[0] = ny * t1[2] - nz * t1[1]; t2[1] = nz * t1[0] - nx * t1[2]; t2[2] = nx * t1[1] - ny * t1[0];
    t1[0] = ny * t2[2] - nz * t2[1]; t1[1] = nz * t2[0] - nx * t2[2]; t1[2] = nx * t2[1] - ny * t2[0];
    double* r = Q.pl[j];
    r[0] = nx; r[1] = ny; r[2] = nz; r[3] = offsets[j]; r[4] = mu[j];
    for (int q = 0; q < 3; q++) { r[5 + q] = t1[q]; r[8 + q] = t2[q]; }
  }
  P = Q;
  return 0;
}

// New offsets for the n colliders in place: 0, or -1 with err naming the collider whose offset is not finite (P untouched)
inline int collider_offsets_validate(const double* offsets, ColliderPlanes& P, std::string& err) {
  char buf[128];
  if (P.n > 0 && !offsets) { err = "null offsets"; return -1; }
  for (int j = 0; j < P.n; j++)
    if (!std::isfinite(offsets[j])) { snprintf(buf, sizeof(buf), "offset %g of collider %d is not finite", offsets[j], j); err = buf; return -1; }
  for (int j = 0; j < P.n; j++) P.pl[j][3] = offsets[j];
  return 0;
}

// The per-vertex mask (NV bytes, bit j: collider j acts on the vertex).  mask == nullptr: every one of the n colliders on every vertex.  -1, naming
// the vertex, for a byte with a bit at or above n (out untouched)
inline int collider_mask_validate(int NV, int32_t n, const uint8_t* mask, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  const unsigned all = n >= 8 ? 0xffu : ((1u << (n > 0 ? n : 0)) - 1u);
  if (!mask) { out.assign((size_t)NV, (uint8_t)all); return 0; }
  for (int v = 0; v < NV; v++)
    if (mask[v] & ~all) { snprintf(buf, sizeof(buf), "mask 0x%02x of vertex %d names a collider at or above %d", (unsigned)mask[v], v, n); err = buf; return -1; }
  out.assign(mask, mask + NV);
  return 0;
}

// The mask from vertex lists, for callers that hold ids: the ids of collider j are ids[ptr[j] .. ptr[j + 1]).  -1, naming collider and vertex, for an
// id outside [0, NV) (out untouched)
inline int collider_mask_from_ids(int NV, int32_t n, const int32_t* ptr, const int32_t* ids, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  std::vector<uint8_t> m((size_t)NV, 0);
  for (int32_t j = 0; j < n && j < TSL_MAX_COLLIDERS; j++)
    for (int32_t e = ptr[j]; e < ptr[j + 1]; e++) {
      const int v = ids[e];
      if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d of collider %d out of range [0, %d)", v, j, NV); err = buf; return -1; }
      m[(size_t)v] |= (uint8_t)(1u << j);
    }
  out.swap(m);
  return 0;
}
