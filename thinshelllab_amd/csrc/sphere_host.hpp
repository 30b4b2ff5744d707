// Host side of the sphere colliders (tsl_set_spheres): the checks of a sphere list and the table as the kernels take it.  Sphere j
// is a solid ball with the cloth outside: a centre c_j that may be set before every step, the previous centre cp_j (where the ball was at the
// start of the step), a radius R_j > 0, fixed once the list is set, and a friction coefficient mu_j >= 0.  Plain C++ with no device code, so that
// it can also be compiled into a stand-alone program (a CPU build under a sanitizer) without the rest of the library, as collider_host.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifndef TSL_MAX_SPHERES
#define TSL_MAX_SPHERES 8
#endif

// The sphere table, passed to every sphere kernel BY VALUE (no global array): row j = (c (3), cp (3), R, mu), 8 doubles.  k: "k_sphere", eps: the
// scene's eps_contact (thickness of the shell), eh: eps_v dt (the friction regularisation of fr_f0 / fr_f1 / fr_f2)
struct SphereTable {
  int n;
  double k, eps, eh;
  double sp[TSL_MAX_SPHERES][8];
};

static inline bool sphere_finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

// 0: the list is valid and S holds it (cp := c; k, eps, eh are left alone).  -1: err names the offender and S is untouched -- more than
// TSL_MAX_SPHERES spheres, a centre that is not finite, a radius that is not finite or <= 0, a friction coefficient that is negative or not finite.
inline int sphere_validate(const double* centres, const double* radii, const double* mu, int32_t n, SphereTable& S, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n > TSL_MAX_SPHERES) { snprintf(buf, sizeof(buf), "%d spheres: at most %d", n, TSL_MAX_SPHERES); err = buf; return -1; }
  if (n > 0 && (!centres || !radii || !mu)) { err = "null centres, null radii or null friction coefficients"; return -1; }
  SphereTable Q = S;
  Q.n = n;
  for (int32_t j = 0; j < TSL_MAX_SPHERES; j++)
    for (int q = 0; q < 8; q++) Q.sp[j][q] = 0.0;
  for (int32_t j = 0; j < n; j++) {
    const double* a = centres + 3 * (size_t)j;
    if (!sphere_finite3(a)) { snprintf(buf, sizeof(buf), "centre (%g, %g, %g) of sphere %d is not finite", a[0], a[1], a[2], j); err = buf; return -1; }
    if (!(std::isfinite(radii[j]) && radii[j] > 0.0)) { snprintf(buf, sizeof(buf), "radius %g of sphere %d is not finite and positive", radii[j], j); err = buf; return -1; }
    if (!(mu[j] >= 0.0 && std::isfinite(mu[j]))) { snprintf(buf, sizeof(buf), "friction coefficient %g of sphere %d is negative or not finite", mu[j], j); err = buf; return -1; }
    double* r = Q.sp[j];
    for (int q = 0; q < 3; q++) { r[q] = a[q]; r[3 + q] = a[q]; }
    r[6] = radii[j]; r[7] = mu[j];
  }
  S = Q;
  return 0;
}

// New centres for the n spheres in place, and their previous centres (prev == nullptr: cp := c): 0, or -1 with err naming the sphere whose centre
// or previous centre is not finite (S untouched)
inline int sphere_centres_validate(const double* centres, const double* prev, SphereTable& S, std::string& err) {
  char buf[256];
  if (S.n > 0 && !centres) { err = "null centres"; return -1; }
  for (int j = 0; j < S.n; j++) {
    const double* a = centres + 3 * (size_t)j;
    if (!sphere_finite3(a)) { snprintf(buf, sizeof(buf), "centre (%g, %g, %g) of sphere %d is not finite", a[0], a[1], a[2], j); err = buf; return -1; }
    if (prev) {
      const double* b = prev + 3 * (size_t)j;
      if (!sphere_finite3(b)) { snprintf(buf, sizeof(buf), "previous centre (%g, %g, %g) of sphere %d is not finite", b[0], b[1], b[2], j); err = buf; return -1; }
    }
  }
  for (int j = 0; j < S.n; j++)
    for (int q = 0; q < 3; q++) {
      S.sp[j][q] = centres[3 * (size_t)j + q];
      S.sp[j][3 + q] = (prev ? prev : centres)[3 * (size_t)j + q];
    }
  return 0;
}

// The per-vertex mask (NV bytes, bit j: sphere j acts on the vertex).  mask == nullptr: every one of the n spheres on every vertex.  -1, naming
// the vertex, for a byte with a bit at or above n (out untouched)
inline int sphere_mask_validate(int NV, int32_t n, const uint8_t* mask, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  const unsigned all = n >= 8 ? 0xffu : ((1u << (n > 0 ? n : 0)) - 1u);
  if (!mask) { out.assign((size_t)NV, (uint8_t)all); return 0; }
  for (int v = 0; v < NV; v++)
    if (mask[v] & ~all) { snprintf(buf, sizeof(buf), "mask 0x%02x of vertex %d names a sphere at or above %d", (unsigned)mask[v], v, n); err = buf; return -1; }
  out.assign(mask, mask + NV);
  return 0;
}

// The mask from vertex lists, for callers that hold ids: the ids of sphere j are ids[ptr[j] .. ptr[j + 1]).  -1, naming sphere and vertex, for an
// id outside [0, NV) (out untouched)
inline int sphere_mask_from_ids(int NV, int32_t n, const int32_t* ptr, const int32_t* ids, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  std::vector<uint8_t> m((size_t)NV, 0);
  for (int32_t j = 0; j < n && j < TSL_MAX_SPHERES; j++)
    for (int32_t e = ptr[j]; e < ptr[j + 1]; e++) {
      const int v = ids[e];
      if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d of sphere %d out of range [0, %d)", v, j, NV); err = buf; return -1; }
      m[(size_t)v] |= (uint8_t)(1u << j);
    }
  out.swap(m);
  return 0;
}
