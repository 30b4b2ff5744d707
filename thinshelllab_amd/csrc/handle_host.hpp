// Host-side check of a handle list (tsl_set_handles): plain C++ with no device code, so that it can also be compiled into a stand-alone
// program (a CPU build under a sanitizer) without the rest of the library.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// 0: the list is valid.  -1: err names the offender -- a vertex outside [0, NV), a vertex with more than one handle (the handle kernels add to a
// vertex's row without atomics: one writer per vertex), a negative or non-finite weight.  weights == nullptr: every weight is 1.
inline int handle_validate(int NV, const int32_t* verts, const double* weights, int32_t n, std::string& err) {
  char buf[256];
  if (n < 0) { snprintf(buf, sizeof(buf), "n = %d is negative", n); err = buf; return -1; }
  if (n == 0) return 0;
  if (!verts) { err = "null vertex list"; return -1; }
  std::vector<unsigned char> seen((size_t)(NV > 0 ? NV : 0), 0);
  for (int32_t i = 0; i < n; i++) {
    const int v = verts[i];
    if (v < 0 || v >= NV) { snprintf(buf, sizeof(buf), "vertex %d out of range [0, %d)", v, NV); err = buf; return -1; }
    if (seen[v]) { snprintf(buf, sizeof(buf), "vertex %d has more than one handle", v); err = buf; return -1; }
    seen[v] = 1;
    if (weights && !(weights[i] >= 0.0 && std::isfinite(weights[i]))) {
      snprintf(buf, sizeof(buf), "weight %g of vertex %d is negative or not finite", weights[i], v); err = buf; return -1;
    }
  }
  return 0;
}
