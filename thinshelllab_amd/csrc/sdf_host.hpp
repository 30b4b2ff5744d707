// Host side of the sampled distance-field colliders (tsl_set_sdfs): the checks of a field list and the table as the kernels take it.
// Field j is a solid {phi < r_j} with the cloth outside, phi the tensor-product uniform cubic B-spline over n0 x n1 x n2 samples (C order, the
// samples are the control values, fixed once the list is set) with one isotropic spacing h_j > 0 and the local position o_j of sample (0, 0, 0); an
// offset r_j (any finite value), a friction coefficient mu_j >= 0, and a pose -- a centre c_j and a quaternion (s, x, y, z) -- that may be set before
// every step, with the previous pose (where the field was at the start of the step).  Quaternions are normalised and turned into rotation matrices
// here, once, by box_pose_check (box_host.hpp).  The count, the friction check and the mask are shape_host.hpp's.  The samples of all fields lie in
// ONE buffer, field j from off[j] on; the table carries the dimensions, the offsets and the buffer's address beside its rows and still goes to the
// kernels by value.  Plain C++ with no device code, so that it can also be compiled into a stand-alone program (a CPU build under a sanitizer)
// without the rest of the library, as box_host.hpp.
// Not modelled: gradients for the samples, a prefilter that makes the spline interpolate, anisotropic spacing, more than SHAPE_MAX fields, any check
// that a solid stays inside its grid (outside 1 <= t < n - 2 a pair contributes nothing: a solid that reaches the border ends there).
#pragma once
#include "box_host.hpp"

// row j = (c (3), R (9, row-major), cp (3), R0 (9), o (3), h, r, mu), 30 doubles.  k: "k_sdf"
enum { SDF_C = 0, SDF_R = 3, SDF_CP = 12, SDF_R0 = 15, SDF_O = 24, SDF_H = 27, SDF_OFF = 28, SDF_MU = 29 };
#define SDF_DIM_MIN 4
#define SDF_DIM_MAX 512
#define SDF_SAMPLES_MAX ((size_t)1 << 26)
struct SdfTable : ShapeTable<30> {
  int32_t dim[SHAPE_MAX][3];   // n0, n1, n2 of field j
  size_t off[SHAPE_MAX];       // its first sample in the buffer
  const double* smp;           // the buffer (device memory in the library; set by the caller of sdf_validate once the samples are uploaded)
};

// 0: the list is valid, S holds it (cp := c, R0 := R; k, eps, eh and smp are left alone) and total is the number of samples, field j at
// samples[S.off[j]].  -1: err names the offender and S is untouched.
inline int sdf_validate(const double* samples, const int32_t* dims, const double* origins, const double* spacings, const double* centres, const double* quats,
                        const double* offsets, const double* mu, int32_t n, SdfTable& S, size_t& total, std::string& err) {
  char buf[256];
  SdfTable Q = S;
  if (shape_count_check<30>("field", n, !samples || !dims || !origins || !spacings || !centres || !quats || !offsets || !mu,
                            "null samples, null dimensions, null origins, null spacings, null centres, null quaternions, null offsets or null friction coefficients", S, Q, err))
    return -1;
  size_t tot = 0;
  for (int32_t j = 0; j < SHAPE_MAX; j++) { Q.dim[j][0] = Q.dim[j][1] = Q.dim[j][2] = 0; Q.off[j] = 0; }
  for (int32_t j = 0; j < n; j++) {
    double* r = Q.row[j];
    const int32_t* d = dims + 3 * (size_t)j;
    for (int a = 0; a < 3; a++)
      if (d[a] < SDF_DIM_MIN || d[a] > SDF_DIM_MAX) {
        snprintf(buf, sizeof(buf), "dimension %d of axis %d of field %d is below %d or above %d", d[a], a, j, SDF_DIM_MIN, SDF_DIM_MAX); err = buf; return -1;
      }
    Q.off[j] = tot;
    tot += (size_t)d[0] * (size_t)d[1] * (size_t)d[2];
    if (tot > SDF_SAMPLES_MAX) { snprintf(buf, sizeof(buf), "%zu samples up to field %d: at most %zu in total", tot, j, SDF_SAMPLES_MAX); err = buf; return -1; }
    for (int a = 0; a < 3; a++) Q.dim[j][a] = d[a];
    if (!(spacings[j] > 0.0) || !std::isfinite(spacings[j])) { snprintf(buf, sizeof(buf), "spacing %g of field %d is not finite and positive", spacings[j], j); err = buf; return -1; }
    const double* o = origins + 3 * (size_t)j;
    if (!finite3(o)) { snprintf(buf, sizeof(buf), "origin (%g, %g, %g) of field %d is not finite", o[0], o[1], o[2], j); err = buf; return -1; }
    if (!std::isfinite(offsets[j])) { snprintf(buf, sizeof(buf), "offset %g of field %d is not finite", offsets[j], j); err = buf; return -1; }
    const std::string bad = box_pose_check("", centres + 3 * (size_t)j, quats + 4 * (size_t)j, j, r + SDF_C, "field");
    if (!bad.empty()) { err = bad; return -1; }
    if (shape_mu_check("field", mu[j], j, err)) return -1;
    for (int q = 0; q < 12; q++) r[SDF_CP + q] = r[SDF_C + q];
    for (int q = 0; q < 3; q++) r[SDF_O + q] = o[q];
    r[SDF_H] = spacings[j]; r[SDF_OFF] = offsets[j]; r[SDF_MU] = mu[j];
  }
  for (int32_t j = 0; j < n; j++) {
    const double* s = samples + Q.off[j];
    const size_t n1 = (size_t)Q.dim[j][1], n2 = (size_t)Q.dim[j][2], cnt = (size_t)Q.dim[j][0] * n1 * n2;
    for (size_t e = 0; e < cnt; e++)
      if (!std::isfinite(s[e])) {
        snprintf(buf, sizeof(buf), "sample (%zu, %zu, %zu) of field %d is not finite (%g)", e / (n1 * n2), (e / n2) % n1, e % n2, j, s[e]); err = buf; return -1;
      }
  }
  S = Q;
  total = tot;
  return 0;
}

// New poses for the n fields in place, and their previous poses (both previous lists nullptr: cp := c, R0 := R; exactly one nullptr is refused): 0,
// or -1 with err naming the field whose centre or previous centre is not finite or whose quaternion or previous quaternion is zero or not finite
// (S untouched)
inline int sdf_poses_validate(const double* centres, const double* quats, const double* prev_centres, const double* prev_quats, SdfTable& S, std::string& err) {
  if (S.n > 0 && (!centres || !quats)) { err = "null centres or null quaternions"; return -1; }
  if ((prev_centres == nullptr) != (prev_quats == nullptr)) { err = prev_centres ? "previous centres without previous quaternions" : "previous quaternions without previous centres"; return -1; }
  double pose[SHAPE_MAX][24];
  for (int j = 0; j < S.n; j++) {
    std::string bad = box_pose_check("", centres + 3 * (size_t)j, quats + 4 * (size_t)j, j, pose[j], "field");
    if (bad.empty()) {
      if (prev_centres) bad = box_pose_check("previous ", prev_centres + 3 * (size_t)j, prev_quats + 4 * (size_t)j, j, pose[j] + 12, "field");
      else for (int q = 0; q < 12; q++) pose[j][12 + q] = pose[j][q];
    }
    if (!bad.empty()) { err = bad; return -1; }
  }
  for (int j = 0; j < S.n; j++)
    for (int q = 0; q < 24; q++) S.row[j][q] = pose[j][q];
  return 0;
}
