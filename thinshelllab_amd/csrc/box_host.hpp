// Host side of the rounded-box colliders (tsl_set_boxes): the checks of a box list and the table as the kernels take it.  Box j is a
// solid box with rounded edges and corners and the cloth outside: a centre c_j and an orientation that may be set before every step, the previous
// pose (where the box was at the start of the step), half extents h_j >= 0 of the core box, a rounding radius r_j > 0 (the solid is the core box
// grown by r_j), both fixed once the list is set, and a friction coefficient mu_j >= 0.  A half extent of 0 is allowed: (L/2, 0, 0) is a rod,
// (0, 0, 0) a ball.  Poses come in as a centre and a quaternion (s, x, y, z); the quaternion is normalised and turned into a rotation matrix here,
// once, with the formula of engine/gripper_single.quat_to_rotmat (frame_host.hpp uses the same): the kernels only ever see matrices.  The
// count, the radius and friction checks and the mask are shape_host.hpp's.  Plain C++ with no device code, so that it can also be compiled into
// a stand-alone program (a CPU build under a sanitizer) without the rest of the library, as capsule_host.hpp.
#pragma once
#include "shape_host.hpp"

// The box table (ShapeTable, shape_host.hpp): row j = (c (3), R (9, row-major: column i is the box axis u_i in the world), cp (3), R0 (9), h (3),
// r, mu), 29 doubles.  k: "k_box"
using BoxTable = ShapeTable<29>;
enum { BOX_C = 0, BOX_R = 3, BOX_CP = 12, BOX_R0 = 15, BOX_H = 24, BOX_RAD = 27, BOX_MU = 28 };

// one pose (what = "" or "previous "): empty and out = (c (3), R (9)), or the message that names the offender (noun: what carries the pose; the
// sampled fields of sdf_host.hpp take the same rule)
static inline std::string box_pose_check(const char* what, const double* c, const double* q, int j, double* out, const char* noun = "box") {
#pragma clang fp contract(off)
  char buf[256];
  if (!finite3(c)) { snprintf(buf, sizeof(buf), "%scentre (%g, %g, %g) of %s %d is not finite", what, c[0], c[1], c[2], noun, j); return buf; }
  const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (!(n > 0.0) || !std::isfinite(n)) {
    snprintf(buf, sizeof(buf), "%squaternion (%g, %g, %g, %g) of %s %d is zero or not finite", what, q[0], q[1], q[2], q[3], noun, j); return buf;
  }
  const double s = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  for (int a = 0; a < 3; a++) out[a] = c[a];
  double* M = out + 3;
  M[0] = s * s + x * x - y * y - z * z; M[1] = 2 * (x * y - s * z);           M[2] = 2 * (x * z + s * y);
  M[3] = 2 * (x * y + s * z);           M[4] = s * s - x * x + y * y - z * z; M[5] = 2 * (y * z - s * x);
  M[6] = 2 * (x * z - s * y);           M[7] = 2 * (y * z + s * x);           M[8] = s * s - x * x - y * y + z * z;
  return std::string();
}

// 0: the list is valid and S holds it (cp := c, R0 := R; k, eps, eh are left alone).  -1: err names the offender and S is untouched -- more than
// SHAPE_MAX boxes, a centre that is not finite, a quaternion that is zero or not finite, a half extent that is negative or not finite, a radius
// that is not finite or <= 0, a friction coefficient that is negative or not finite.
inline int box_validate(const double* centres, const double* quats, const double* half, const double* radii, const double* mu, int32_t n, BoxTable& S, std::string& err) {
  char buf[256];
  BoxTable Q;
  if (n > SHAPE_MAX) { snprintf(buf, sizeof(buf), "%d boxes: at most %d", n, SHAPE_MAX); err = buf; return -1; }
  if (shape_count_check("box", n, !centres || !quats || !half || !radii || !mu, "null centres, null quaternions, null half extents, null radii or null friction coefficients", S, Q, err)) return -1;
  for (int32_t j = 0; j < n; j++) {
    double* r = Q.row[j];
    const std::string bad = box_pose_check("", centres + 3 * (size_t)j, quats + 4 * (size_t)j, j, r + BOX_C);
    if (!bad.empty()) { err = bad; return -1; }
    const double* hj = half + 3 * (size_t)j;
    if (!finite3(hj) || !(hj[0] >= 0.0 && hj[1] >= 0.0 && hj[2] >= 0.0)) {
      snprintf(buf, sizeof(buf), "half extents (%g, %g, %g) of box %d are negative or not finite", hj[0], hj[1], hj[2], j); err = buf; return -1;
    }
    if (shape_radius_check("box", radii[j], j, err) || shape_mu_check("box", mu[j], j, err)) return -1;
    for (int q = 0; q < 12; q++) r[BOX_CP + q] = r[BOX_C + q];
    for (int q = 0; q < 3; q++) r[BOX_H + q] = hj[q];
    r[BOX_RAD] = radii[j]; r[BOX_MU] = mu[j];
  }
  S = Q;
  return 0;
}

// New poses for the n boxes in place, and their previous poses (both previous lists nullptr: cp := c, R0 := R; exactly one nullptr is refused): 0, or
// -1 with err naming the box whose centre or previous centre is not finite or whose quaternion or previous quaternion is zero or not finite (S
// untouched)
inline int box_poses_validate(const double* centres, const double* quats, const double* prev_centres, const double* prev_quats, BoxTable& S, std::string& err) {
  if (S.n > 0 && (!centres || !quats)) { err = "null centres or null quaternions"; return -1; }
  if ((prev_centres == nullptr) != (prev_quats == nullptr)) { err = prev_centres ? "previous centres without previous quaternions" : "previous quaternions without previous centres"; return -1; }
  double pose[SHAPE_MAX][24];
  for (int j = 0; j < S.n; j++) {
    std::string bad = box_pose_check("", centres + 3 * (size_t)j, quats + 4 * (size_t)j, j, pose[j]);
    if (bad.empty()) {
      if (prev_centres) bad = box_pose_check("previous ", prev_centres + 3 * (size_t)j, prev_quats + 4 * (size_t)j, j, pose[j] + 12);
      else for (int q = 0; q < 12; q++) pose[j][12 + q] = pose[j][q];
    }
    if (!bad.empty()) { err = bad; return -1; }
  }
  for (int j = 0; j < S.n; j++)
    for (int q = 0; q < 24; q++) S.row[j][q] = pose[j][q];
  return 0;
}
