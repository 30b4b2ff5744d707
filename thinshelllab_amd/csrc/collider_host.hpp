// Host side of the half-space colliders (tsl_set_colliders): the checks of a collider list and the plane table as the kernels take
// it.  Collider j is the half-space n_j . x < o_j (the solid side) with a unit normal n_j, fixed once the list is set, an offset o_j that may be
// set before every step, and a friction coefficient mu_j >= 0.  The count, the friction check and the mask are shape_host.hpp's.  Plain C++ with
// no device code, so that it can also be compiled into a stand-alone program (a CPU build under a sanitizer) without the rest of the library, as
// tie_host.hpp.
#pragma once
#include "shape_host.hpp"

// The plane table (ShapeTable, shape_host.hpp): row j = (n (3), o, mu, t1 (3), t2 (3)), 11 doubles.  k: "k_collider"
using ColliderPlanes = ShapeTable<11>;

// 0: the list is valid and P holds it (normals normalised, the tangent pair T = (t1, t2) built from the unit normal exactly as k_contact_pair builds
// c_T; k, eps, eh are left alone).  -1: err names the offender and P is untouched -- more than SHAPE_MAX colliders, a normal that is
// zero or not finite, an offset that is not finite, a friction coefficient that is negative or not finite.
inline int collider_validate(const double* normals, const double* offsets, const double* mu, int32_t n, ColliderPlanes& P, std::string& err) {
  char buf[256];
  ColliderPlanes Q;
  if (shape_count_check("collider", n, !normals || !offsets || !mu, "null normals, null offsets or null friction coefficients", P, Q, err)) return -1;
  for (int32_t j = 0; j < n; j++) {
    const double* a = normals + 3 * (size_t)j;
    const double len = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if (!(std::isfinite(len) && len > 0.0)) {
      snprintf(buf, sizeof(buf), "normal (%g, %g, %g) of collider %d is zero or not finite", a[0], a[1], a[2], j); err = buf; return -1;
    }
    if (!std::isfinite(offsets[j])) { snprintf(buf, sizeof(buf), "offset %g of collider %d is not finite", offsets[j], j); err = buf; return -1; }
    if (shape_mu_check("collider", mu[j], j, err)) return -1;
    const double nx = a[0] / len, ny = a[1] / len, nz = a[2] / len;
    // t1 = |n.x| < 0.5 ? (n.x, n.z, -n.y) : (n.y, -n.x, n.z);  t2 = n x t1;  t1 = n x t2   (k_contact_pair)
    double t1[3], t2[3];
    if (std::fabs(nx) < 0.5) { t1[0] = nx; t1[1] = nz; t1[2] = -ny; } else { t1[0] = ny; t1[1] = -nx; t1[2] = nz; }
    t2[0] = ny * t1[2] - nz * t1[1]; t2[1] = nz * t1[0] - nx * t1[2]; t2[2] = nx * t1[1] - ny * t1[0];
    t1[0] = ny * t2[2] - nz * t2[1]; t1[1] = nz * t2[0] - nx * t2[2]; t1[2] = nx * t2[1] - ny * t2[0];
    double* r = Q.row[j];
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
  for (int j = 0; j < P.n; j++) P.row[j][3] = offsets[j];
  return 0;
}
