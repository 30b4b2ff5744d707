// Test program (never part of libtsl_hip.so): the checks and the sphere table of csrc/sphere_host.hpp, printed as "name: numbers" lines for
// tests/test_sphere_numpy.py, which builds it with -fsanitize=address,undefined.  The refused lists print "refused: <message>"; the program ends
// with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/sphere_host.hpp"

template <class T>
static void show(const char* name, const std::vector<T>& a) {
  printf("%s:", name);
  for (T x : a) printf(" %.17g", (double)x);
  printf("\n");
}
static std::vector<double> table(const SphereTable& S) {
  std::vector<double> t;
  for (int j = 0; j < S.n; j++) t.insert(t.end(), S.row[j], S.row[j] + 8);
  return t;
}

int main() {
  const int NV = 20;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string err;
  // a valid list of three balls
  const std::vector<double> cen = {0.0, 0.0, -0.05,  0.01, -0.02, 0.03,  -3.0, 0.5, 0.25};
  const std::vector<double> rad = {0.05, 0.002, 1.0e4}, mu = {0.0, 0.4, 1.5};
  SphereTable S{};
  S.k = 7.0; S.eps = 0.5; S.eh = 0.25;
  if (sphere_validate(cen.data(), rad.data(), mu.data(), 3, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("centres", cen); show("radii", rad); show("mu", mu);
  show("table", table(S));
  show("scalars", std::vector<double>{(double)S.n, S.k, S.eps, S.eh});
  const std::vector<double> keep = table(S);

  // the refused lists: one offender each, behind a valid ball; the list in place stays
  struct Bad { double c[3], R, mu; };
  const Bad bad[] = {{{nan, 0.0, 1.0}, 0.1, 0.1}, {{0.0, inf, 1.0}, 0.1, 0.1}, {{0.0, 0.0, -inf}, 0.1, 0.1}, {{0.0, 0.0, 1.0}, 0.0, 0.1},
                     {{0.0, 0.0, 1.0}, -0.1, 0.1}, {{0.0, 0.0, 1.0}, nan, 0.1}, {{0.0, 0.0, 1.0}, inf, 0.1}, {{0.0, 0.0, 1.0}, 0.1, -0.5},
                     {{0.0, 0.0, 1.0}, 0.1, nan}, {{0.0, 0.0, 1.0}, 0.1, inf}};
  int kept = 1;
  for (const Bad& q : bad) {
    const std::vector<double> c2 = {0.0, 0.0, 1.0, q.c[0], q.c[1], q.c[2]}, r2 = {1.0, q.R}, m2 = {0.0, q.mu};
    err.clear();
    const int rc = sphere_validate(c2.data(), r2.data(), m2.data(), 2, S, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
  }
  {   // nine spheres; a negative count
    const std::vector<double> c9(27, 1.0), r9(9, 1.0), m9(9, 0.0);
    err.clear();
    printf("refused: %s\n", sphere_validate(c9.data(), r9.data(), m9.data(), 9, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    err.clear();
    printf("refused: %s\n", sphere_validate(c9.data(), r9.data(), m9.data(), -1, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    // eight are the most
    SphereTable S8{};
    if (sphere_validate(c9.data(), r9.data(), m9.data(), 8, S8, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    printf("eight: %d\n", S8.n);
  }
  // centres alone: a non-finite centre, a non-finite previous centre, both given, the previous ones left out
  {
    std::vector<double> c3 = cen, p3 = cen;
    c3[4] = nan;
    err.clear();
    printf("refused: %s\n", sphere_centres_validate(c3.data(), nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    c3[4] = 0.125; p3[8] = inf;
    err.clear();
    printf("refused: %s\n", sphere_centres_validate(c3.data(), p3.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    p3[8] = -0.75;
    if (sphere_centres_validate(c3.data(), p3.data(), S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("moved_c", c3); show("moved_cp", p3);
    show("table_moved", table(S));
    if (sphere_centres_validate(c3.data(), nullptr, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("table_at_rest", table(S));
  }
  // masks: the default, a given one, a bit at or above n; vertex lists, an id out of range
  std::vector<uint8_t> mask, mask0;
  if (shape_mask_validate("sphere", NV, 3, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_all", mask);
  mask0 = mask;
  std::vector<uint8_t> given(NV, 5); given[7] = 0; given[9] = 8;
  err.clear();
  printf("refused: %s\n", shape_mask_validate("sphere", NV, 3, given.data(), mask, err) ? err.c_str() : "NOT REFUSED");
  kept &= (mask == mask0);
  given[9] = 2;
  if (shape_mask_validate("sphere", NV, 3, given.data(), mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_given", mask);
  if (shape_mask_validate("sphere", NV, 8, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_eight", mask);
  const std::vector<int32_t> ptr = {0, 3, 3, 5};
  std::vector<int32_t> ids = {0, 19, 4, 4, 5};
  if (shape_mask_from_ids("sphere", NV, 3, ptr.data(), ids.data(), mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_ids", mask);
  mask0 = mask;
  for (int32_t wrong : {NV, -1}) {
    ids[4] = wrong;
    err.clear();
    printf("refused: %s\n", shape_mask_from_ids("sphere", NV, 3, ptr.data(), ids.data(), mask, err) ? err.c_str() : "NOT REFUSED");
    kept &= (mask == mask0);
  }
  // no spheres: valid, an empty table
  SphereTable E{};
  if (sphere_validate(nullptr, nullptr, nullptr, 0, E, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  printf("empty: %d\n", E.n);
  printf("kept: %d\n", kept);
  printf("done\n");
  return 0;
}
