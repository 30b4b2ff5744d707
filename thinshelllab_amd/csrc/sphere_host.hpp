// Host side of the sphere colliders (tsl_set_spheres): the checks of a sphere list and the table as the kernels take it.  Sphere j
// is a solid ball with the cloth outside: a centre c_j that may be set before every step, the previous centre cp_j (where the ball was at the
// start of the step), a radius R_j > 0, fixed once the list is set, and a friction coefficient mu_j >= 0.  The count, the radius and friction
// checks and the mask are shape_host.hpp's.  Plain C++ with no device code, so that it can also be compiled into a stand-alone program (a CPU
// build under a sanitizer) without the rest of the library, as collider_host.hpp.
#pragma once
#include "shape_host.hpp"

// The sphere table (ShapeTable, shape_host.hpp): row j = (c (3), cp (3), R, mu), 8 doubles.  k: "k_sphere"
using SphereTable = ShapeTable<8>;

// 0: the list is valid and S holds it (cp := c; k, eps, eh are left alone).  -1: err names the offender and S is untouched -- more than
// SHAPE_MAX spheres, a centre that is not finite, a radius that is not finite or <= 0, a friction coefficient that is negative or not finite.
inline int sphere_validate(const double* centres, const double* radii, const double* mu, int32_t n, SphereTable& S, std::string& err) {
  char buf[256];
  SphereTable Q;
  if (shape_count_check("sphere", n, !centres || !radii || !mu, "null centres, null radii or null friction coefficients", S, Q, err)) return -1;
  for (int32_t j = 0; j < n; j++) {
    const double* a = centres + 3 * (size_t)j;
    if (!finite3(a)) { snprintf(buf, sizeof(buf), "centre (%g, %g, %g) of sphere %d is not finite", a[0], a[1], a[2], j); err = buf; return -1; }
    if (shape_radius_check("sphere", radii[j], j, err) || shape_mu_check("sphere", mu[j], j, err)) return -1;
    double* r = Q.row[j];
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
    if (!finite3(a)) { snprintf(buf, sizeof(buf), "centre (%g, %g, %g) of sphere %d is not finite", a[0], a[1], a[2], j); err = buf; return -1; }
    if (prev) {
      const double* b = prev + 3 * (size_t)j;
      if (!finite3(b)) { snprintf(buf, sizeof(buf), "previous centre (%g, %g, %g) of sphere %d is not finite", b[0], b[1], b[2], j); err = buf; return -1; }
    }
  }
  for (int j = 0; j < S.n; j++)
    for (int q = 0; q < 3; q++) {
      S.row[j][q] = centres[3 * (size_t)j + q];
      S.row[j][3 + q] = (prev ? prev : centres)[3 * (size_t)j + q];
    }
  return 0;
}
