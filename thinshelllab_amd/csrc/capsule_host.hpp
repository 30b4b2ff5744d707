// Host side of the capsule colliders (tsl_set_capsules): the checks of a capsule list and the table as the kernels take it.  Capsule j
// is a solid rod with round ends and the cloth outside: endpoints a_j, b_j that may be set before every step, the previous endpoints ap_j, bp_j
// (where the rod was at the start of the step), a radius R_j > 0, fixed once the list is set, and a friction coefficient mu_j >= 0.  The endpoints
// move independently (the rod may translate, rotate and change its length); a segment shorter than CAPSULE_MIN_LEN is refused -- a ball is what
// tsl_set_spheres is for.  Plain C++ with no device code, so that it can also be compiled into a stand-alone program (a CPU build under a
// sanitizer) without the rest of the library, as sphere_host.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifndef TSL_MAX_CAPSULES
#define TSL_MAX_CAPSULES 8
#endif
#define CAPSULE_MIN_LEN 1e-9   // metres

// The capsule table, passed to every capsule kernel BY VALUE (no global array): row j = (a (3), b (3), ap (3), bp (3), R, mu), 14 doubles.  k:
// "k_capsule", eps: the scene's eps_contact (thickness of the shell), eh: eps_v dt (the friction regularisation of fr_f0 / fr_f1 / fr_f2)
struct CapsuleTable {
  int n;
  double k, eps, eh;
  double cp[TSL_MAX_CAPSULES][14];
};

static inline bool capsule_finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }
static inline double capsule_len(const double* a, const double* b) {
  const double x = b[0] - a[0], y = b[1] - a[1], z = b[2] - a[2];
  return std::sqrt(x * x + y * y + z * z);
}
// the two endpoints of one state (what = "" or "previous "): empty, or the message that names the offender
static inline std::string capsule_ends_check(const char* what, const double* a, const double* b, int j) {
  char buf[256];
  if (!capsule_finite3(a)) { snprintf(buf, sizeof(buf), "%sendpoint a (%g, %g, %g) of capsule %d is not finite", what, a[0], a[1], a[2], j); return buf; }
  if (!capsule_finite3(b)) { snprintf(buf, sizeof(buf), "%sendpoint b (%g, %g, %g) of capsule %d is not finite", what, b[0], b[1], b[2], j); return buf; }
  const double len = capsule_len(a, b);
  if (!(len >= CAPSULE_MIN_LEN)) { snprintf(buf, sizeof(buf), "%ssegment of capsule %d is %g m long: at least %g m", what, j, len, CAPSULE_MIN_LEN); return buf; }
  return std::string();
}

// 0: the list is valid and S holds it (ap := a, bp := b; k, eps, eh are left alone).  -1: err names the offender and S is untouched -- more than
// TSL_MAX_CAPSULES capsules, an endpoint that is not finite, a segment shorter than CAPSULE_MIN_LEN, a radius that is not finite or <= 0, a
// friction coefficient that is negative or not finite.
inline int capsule_validate(const double* a, const double* b, const double* radii, const double* mu, int32_t n, CapsuleTable& S, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n > TSL_MAX_CAPSULES) { snprintf(buf, sizeof(buf), "%d capsules: at most %d", n, TSL_MAX_CAPSULES); err = buf; return -1; }
  if (n > 0 && (!a || !b || !radii || !mu)) { err = "null endpoints, null radii or null friction coefficients"; return -1; }
  CapsuleTable Q = S;
  Q.n = n;
  for (int32_t j = 0; j < TSL_MAX_CAPSULES; j++)
    for (int q = 0; q < 14; q++) Q.cp[j][q] = 0.0;
  for (int32_t j = 0; j < n; j++) {
    const double* aj = a + 3 * (size_t)j;
    const double* bj = b + 3 * (size_t)j;
    const std::string bad = capsule_ends_check("", aj, bj, j);
    if (!bad.empty()) { err = bad; return -1; }
    if (!(std::isfinite(radii[j]) && radii[j] > 0.0)) { snprintf(buf, sizeof(buf), "radius %g of capsule %d is not finite and positive", radii[j], j); err = buf; return -1; }
    if (!(mu[j] >= 0.0 && std::isfinite(mu[j]))) { snprintf(buf, sizeof(buf), "friction coefficient %g of capsule %d is negative or not finite", mu[j], j); err = buf; return -1; }
    double* r = Q.cp[j];
    for (int q = 0; q < 3; q++) { r[q] = aj[q]; r[3 + q] = bj[q]; r[6 + q] = aj[q]; r[9 + q] = bj[q]; }
    r[12] = radii[j]; r[13] = mu[j];
  }
  S = Q;
  return 0;
}

// New endpoints for the n capsules in place, and their previous endpoints (both nullptr: ap := a, bp := b; exactly one nullptr is refused): 0, or -1
// with err naming the capsule whose endpoint or previous endpoint is not finite or whose segment or previous segment is too short (S untouched)
inline int capsule_ends_validate(const double* a, const double* b, const double* prev_a, const double* prev_b, CapsuleTable& S, std::string& err) {
  if (S.n > 0 && (!a || !b)) { err = "null endpoints"; return -1; }
  if ((prev_a == nullptr) != (prev_b == nullptr)) { err = prev_a ? "previous endpoints a without previous endpoints b" : "previous endpoints b without previous endpoints a"; return -1; }
  for (int j = 0; j < S.n; j++) {
    std::string bad = capsule_ends_check("", a + 3 * (size_t)j, b + 3 * (size_t)j, j);
    if (bad.empty() && prev_a) bad = capsule_ends_check("previous ", prev_a + 3 * (size_t)j, prev_b + 3 * (size_t)j, j);
    if (!bad.empty()) { err = bad; return -1; }
  }
  for (int j = 0; j < S.n; j++)
    for (int q = 0; q < 3; q++) {
      S.cp[j][q] = a[3 * (size_t)j + q];
      S.cp[j][3 + q] = b[3 * (size_t)j + q];
      S.cp[j][6 + q] = (prev_a ? prev_a : a)[3 * (size_t)j + q];
      S.cp[j][9 + q] = (prev_b ? prev_b : b)[3 * (size_t)j + q];
    }
  return 0;
}

// The per-vertex mask (NV bytes, bit j: capsule j acts on the vertex).  mask == nullptr: every one of the n capsules on every vertex.  -1, naming
// the vertex, for a byte with a bit at or above n (out untouched)
inline int capsule_mask_validate(int NV, int32_t n, const uint8_t* mask, std::vector<uint8_t>& out, std::string& err) {
  char buf[128];
  const unsigned all = n >= 8 ? 0xffu : ((1u << (n > 0 ? n : 0)) - 1u);
  if (!mask) { out.assign((size_t)NV, (uint8_t)all); return 0; }
  for (int v = 0; v < NV; v++)
    if (mask[v] & ~all) { snprintf(buf, sizeof(buf), "mask 0x%02x of vertex %d names a capsule at or above %d", (unsigned)mask[v], v, n); err = buf; return -1; }
  out.assign(mask, mask + NV);
  return 0;
}
