// Host side of the capsule colliders (tsl_set_capsules): the checks of a capsule list and the table as the kernels take it.  Capsule j
// is a solid rod with round ends and the cloth outside: endpoints a_j, b_j that may be set before every step, the previous endpoints ap_j, bp_j
// (where the rod was at the start of the step), a radius R_j > 0, fixed once the list is set, and a friction coefficient mu_j >= 0.  The endpoints
// move independently (the rod may translate, rotate and change its length); a segment shorter than CAPSULE_MIN_LEN is refused -- a ball is what
// tsl_set_spheres is for.  The count, the radius and friction checks and the mask are shape_host.hpp's.  Plain C++ with no device code, so that
// it can also be compiled into a stand-alone program (a CPU build under a sanitizer) without the rest of the library, as sphere_host.hpp.
#pragma once
#include "shape_host.hpp"

#define CAPSULE_MIN_LEN 1e-9   // metres

// The capsule table (ShapeTable, shape_host.hpp): row j = (a (3), b (3), ap (3), bp (3), R, mu), 14 doubles.  k: "k_capsule"
using CapsuleTable = ShapeTable<14>;

static inline double capsule_len(const double* a, const double* b) {
  const double x = b[0] - a[0], y = b[1] - a[1], z = b[2] - a[2];
  return std::sqrt(x * x + y * y + z * z);
}
// the two endpoints of one state (what = "" or "previous "): empty, or the message that names the offender
static inline std::string capsule_ends_check(const char* what, const double* a, const double* b, int j) {
  char buf[256];
  if (!finite3(a)) { snprintf(buf, sizeof(buf), "%sendpoint a (%g, %g, %g) of capsule %d is not finite", what, a[0], a[1], a[2], j); return buf; }
  if (!finite3(b)) { snprintf(buf, sizeof(buf), "%sendpoint b (%g, %g, %g) of capsule %d is not finite", what, b[0], b[1], b[2], j); return buf; }
  const double len = capsule_len(a, b);
  if (!(len >= CAPSULE_MIN_LEN)) { snprintf(buf, sizeof(buf), "%ssegment of capsule %d is %g m long: at least %g m", what, j, len, CAPSULE_MIN_LEN); return buf; }
  return std::string();
}

// 0: the list is valid and S holds it (ap := a, bp := b; k, eps, eh are left alone).  -1: err names the offender and S is untouched -- more than
// SHAPE_MAX capsules, an endpoint that is not finite, a segment shorter than CAPSULE_MIN_LEN, a radius that is not finite or <= 0, a
// friction coefficient that is negative or not finite.
inline int capsule_validate(const double* a, const double* b, const double* radii, const double* mu, int32_t n, CapsuleTable& S, std::string& err) {
  CapsuleTable Q;
  if (shape_count_check("capsule", n, !a || !b || !radii || !mu, "null endpoints, null radii or null friction coefficients", S, Q, err)) return -1;
  for (int32_t j = 0; j < n; j++) {
    const double* aj = a + 3 * (size_t)j;
    const double* bj = b + 3 * (size_t)j;
    const std::string bad = capsule_ends_check("", aj, bj, j);
    if (!bad.empty()) { err = bad; return -1; }
    if (shape_radius_check("capsule", radii[j], j, err) || shape_mu_check("capsule", mu[j], j, err)) return -1;
    double* r = Q.row[j];
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
      S.row[j][q] = a[3 * (size_t)j + q];
      S.row[j][3 + q] = b[3 * (size_t)j + q];
      S.row[j][6 + q] = (prev_a ? prev_a : a)[3 * (size_t)j + q];
      S.row[j][9 + q] = (prev_b ? prev_b : b)[3 * (size_t)j + q];
    }
  return 0;
}
