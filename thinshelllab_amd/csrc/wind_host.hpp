// Host side of the wind (tsl_set_wind, tsl_set_wind_velocity): the checks of the face list and of the wind velocity.  Plain C++
// with no device code, so that it can also be compiled into a stand-alone program (a CPU build under a sanitizer) without the rest of the library.
// The gather lists of the wind kernels (k_wind.hpp) are those of a face list of handles: handle_lists(pattern, corners, n, 3, ...) of handle_host.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// A wind list: n faces of the scene's global face table, whose first n_cface faces are the cloths' and whose faces [n_cface, NF) are the surface
// faces of the FEM bodies.  0: the list is valid.  -1: err names the offender -- a negative n, a face outside [0, NF), a surface face of a body
// (the drag of a volume is not this model), a face listed twice (its drag would count twice: use the weight), a negative or non-finite weight.
// weights == nullptr: every weight is 1.
inline int wind_validate(int n_cface, int NF, const int32_t* faces, const double* weights, int32_t n, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n == 0) return 0;
  if (n >= (1 << 27)) { snprintf(buf, sizeof(buf), "n = %d: too many faces for the packed gather lists", n); err = buf; return -1; }
  if (!faces) { err = "null face list"; return -1; }
  std::vector<int32_t> first((size_t)(n_cface > 0 ? n_cface : 0), -1);   // entry that listed the face first
  for (int32_t i = 0; i < n; i++) {
    const int f = faces[i];
    if (f < 0 || f >= NF) { snprintf(buf, sizeof(buf), "face %d of entry %d out of range [0, %d)", f, i, NF); err = buf; return -1; }
    if (f >= n_cface) {
      snprintf(buf, sizeof(buf), "face %d of entry %d is a surface face of a body, not a cloth face (cloth faces are [0, %d))", f, i, n_cface); err = buf; return -1;
    }
    if (first[f] >= 0) { snprintf(buf, sizeof(buf), "face %d is listed twice (entries %d and %d)", f, first[f], i); err = buf; return -1; }
    first[f] = i;
    if (weights && !(weights[i] >= 0.0 && std::isfinite(weights[i]))) {
      snprintf(buf, sizeof(buf), "weight %g of entry %d (face %d) is negative or not finite", weights[i], i, f); err = buf; return -1;
    }
  }
  return 0;
}

// The wind velocity of the next step.  0: W (3 values) is finite and copied to out.  -1: err names the component; out is left as it was.
inline int wind_velocity_validate(const double* W, double* out, std::string& err) {
  char buf[256];
  if (!W) { err = "null wind velocity"; return -1; }
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(W[a])) { snprintf(buf, sizeof(buf), "component %d of the wind velocity (%g, %g, %g) is not finite", a, W[0], W[1], W[2]); err = buf; return -1; }
  for (int a = 0; a < 3; a++) out[a] = W[a];
  return 0;
}
