// Test program (never part of libtsl_hip.so): the checks and the plane table of csrc/collider_host.hpp, printed as "name: numbers" lines for
// tests/test_collider_numpy.py, which builds it with -fsanitize=address,undefined.  The refused lists print "refused: <message>"; the program ends
// with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/collider_host.hpp"

template <class T>
static void show(const char* name, const std::vector<T>& a) {
  printf("%s:", name);
  for (T x : a) printf(" %.17g", (double)x);
  printf("\n");
}
static std::vector<double> table(const ColliderPlanes& P) {
  std::vector<double> t;
  for (int j = 0; j < P.n; j++) t.insert(t.end(), P.row[j], P.row[j] + 11);
  return t;
}

int main() {
  const int NV = 20;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string err;
  // a valid list: a floor, a tilted plane (|n.x| < 0.5), a wall (|n.x| >= 0.5), normals of any length
  const std::vector<double> nrm = {0.0, 0.0, 2.0,  0.0, 0.3, 1.0,  -3.0, 0.5, 0.25};
  const std::vector<double> off = {-0.01, 0.02, -1.5}, mu = {0.0, 0.4, 1.5};
  ColliderPlanes P{};
  P.k = 7.0; P.eps = 0.5; P.eh = 0.25;
  if (collider_validate(nrm.data(), off.data(), mu.data(), 3, P, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("normals", nrm); show("offsets", off); show("mu", mu);
  show("table", table(P));
  show("scalars", std::vector<double>{(double)P.n, P.k, P.eps, P.eh});
  const std::vector<double> keep = table(P);

  // the refused lists: one offender each, behind a valid collider; the list in place stays
  struct Bad { double n[3], o, mu; };
  const Bad bad[] = {{{0.0, 0.0, 0.0}, 0.0, 0.1}, {{nan, 0.0, 1.0}, 0.0, 0.1}, {{0.0, inf, 1.0}, 0.0, 0.1}, {{0.0, 0.0, 1.0}, nan, 0.1},
                     {{0.0, 0.0, 1.0}, -inf, 0.1}, {{0.0, 0.0, 1.0}, 0.0, -0.5}, {{0.0, 0.0, 1.0}, 0.0, nan}, {{0.0, 0.0, 1.0}, 0.0, inf}};
  int kept = 1;
  for (const Bad& q : bad) {
    const std::vector<double> n2 = {0.0, 0.0, 1.0, q.n[0], q.n[1], q.n[2]}, o2 = {0.0, q.o}, m2 = {0.0, q.mu};
    err.clear();
    const int rc = collider_validate(n2.data(), o2.data(), m2.data(), 2, P, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
    kept &= (table(P) == keep && P.n == 3);
  }
  {   // nine colliders; a negative count
    const std::vector<double> n9(27, 1.0), o9(9, 0.0), m9(9, 0.0);
    err.clear();
    printf("refused: %s\n", collider_validate(n9.data(), o9.data(), m9.data(), 9, P, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(P) == keep && P.n == 3);
    err.clear();
    printf("refused: %s\n", collider_validate(n9.data(), o9.data(), m9.data(), -1, P, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(P) == keep && P.n == 3);
    // eight are the most
    ColliderPlanes P8{};
    if (collider_validate(n9.data(), o9.data(), m9.data(), 8, P8, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    printf("eight: %d\n", P8.n);
  }
  // offsets alone
  {
    const std::vector<double> o3 = {0.1, nan, 0.3};
    err.clear();
    printf("refused: %s\n", collider_offsets_validate(o3.data(), P, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(P) == keep);
    const std::vector<double> o4 = {0.1, 0.2, 0.3};
    if (collider_offsets_validate(o4.data(), P, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("table_moved", table(P));
  }
  // masks: the default, a given one, a bit at or above n; vertex lists, an id out of range
  std::vector<uint8_t> mask, mask0;
  if (shape_mask_validate("collider", NV, 3, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_all", mask);
  mask0 = mask;
  std::vector<uint8_t> given(NV, 5); given[7] = 0; given[9] = 8;
  err.clear();
  printf("refused: %s\n", shape_mask_validate("collider", NV, 3, given.data(), mask, err) ? err.c_str() : "NOT REFUSED");
  kept &= (mask == mask0);
  given[9] = 2;
  if (shape_mask_validate("collider", NV, 3, given.data(), mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_given", mask);
  const std::vector<int32_t> ptr = {0, 3, 3, 5};
  std::vector<int32_t> ids = {0, 19, 4, 4, 5};
  if (shape_mask_from_ids("collider", NV, 3, ptr.data(), ids.data(), mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_ids", mask);
  mask0 = mask;
  for (int32_t wrong : {NV, -1}) {
    ids[4] = wrong;
    err.clear();
    printf("refused: %s\n", shape_mask_from_ids("collider", NV, 3, ptr.data(), ids.data(), mask, err) ? err.c_str() : "NOT REFUSED");
    kept &= (mask == mask0);
  }
  // no colliders: valid, an empty table
  ColliderPlanes E{};
  if (collider_validate(nullptr, nullptr, nullptr, 0, E, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  printf("empty: %d\n", E.n);
  printf("kept: %d\n", kept);
  printf("done\n");
  return 0;
}
