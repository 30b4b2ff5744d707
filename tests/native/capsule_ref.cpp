// Test program (never part of libtsl_hip.so): the checks and the capsule table of csrc/capsule_host.hpp, printed as "name: numbers" lines for
// tests/test_capsule_numpy.py, which builds it with -fsanitize=address,undefined.  The refused lists print "refused: <message>"; the program ends
// with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/capsule_host.hpp"

template <class T>
static void show(const char* name, const std::vector<T>& a) {
  printf("%s:", name);
  for (T x : a) printf(" %.17g", (double)x);
  printf("\n");
}
static std::vector<double> table(const CapsuleTable& S) {
  std::vector<double> t;
  for (int j = 0; j < S.n; j++) t.insert(t.end(), S.row[j], S.row[j] + 14);
  return t;
}

int main() {
  const int NV = 20;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string err;
  // a valid list of three rods
  const std::vector<double> A = {-0.02, 0.0, -0.005,  0.01, -0.02, 0.03,  -3.0, 0.5, 0.25};
  const std::vector<double> B = {0.02, 0.0, -0.005,  0.01, -0.02, 0.03 + 2e-9,  4.0, 0.5, 0.25};
  const std::vector<double> rad = {0.005, 0.002, 1.0e4}, mu = {0.0, 0.4, 1.5};
  CapsuleTable S{};
  S.k = 7.0; S.eps = 0.5; S.eh = 0.25;
  if (capsule_validate(A.data(), B.data(), rad.data(), mu.data(), 3, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("a", A); show("b", B); show("radii", rad); show("mu", mu);
  show("table", table(S));
  show("scalars", std::vector<double>{(double)S.n, S.k, S.eps, S.eh});
  const std::vector<double> keep = table(S);

  // the refused lists: one offender each, behind a valid rod; the list in place stays
  struct Bad { double a[3], b[3], R, mu; };
  const Bad bad[] = {{{nan, 0.0, 1.0}, {1.0, 0.0, 1.0}, 0.1, 0.1}, {{0.0, 0.0, 1.0}, {1.0, inf, 1.0}, 0.1, 0.1}, {{0.0, 0.0, -inf}, {1.0, 0.0, 1.0}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {0.0, 0.0, 1.0}, 0.1, 0.1}, {{0.0, 0.0, 1.0}, {0.0, 5e-10, 1.0}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, 0.0, 0.1}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, -0.1, 0.1}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, nan, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, inf, 0.1}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, 0.1, -0.5}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, 0.1, nan},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 1.0}, 0.1, inf}};
  int kept = 1;
  for (const Bad& q : bad) {
    const std::vector<double> a2 = {0.0, 0.0, 1.0, q.a[0], q.a[1], q.a[2]}, b2 = {0.0, 1.0, 1.0, q.b[0], q.b[1], q.b[2]}, r2 = {1.0, q.R}, m2 = {0.0, q.mu};
    err.clear();
    const int rc = capsule_validate(a2.data(), b2.data(), r2.data(), m2.data(), 2, S, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
  }
  {   // nine capsules; a negative count
    std::vector<double> a9(27, 1.0), b9(27, 2.0), r9(9, 1.0), m9(9, 0.0);
    err.clear();
    printf("refused: %s\n", capsule_validate(a9.data(), b9.data(), r9.data(), m9.data(), 9, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    err.clear();
    printf("refused: %s\n", capsule_validate(a9.data(), b9.data(), r9.data(), m9.data(), -1, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    // eight are the most
    CapsuleTable S8{};
    if (capsule_validate(a9.data(), b9.data(), r9.data(), m9.data(), 8, S8, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    printf("eight: %d\n", S8.n);
  }
  // endpoints alone: a non-finite endpoint, a short segment, a non-finite previous endpoint, a short previous segment, one previous list without the
  // other; then all four given, then the previous ones left out
  {
    std::vector<double> a3 = A, b3 = B, pa = A, pb = B;
    a3[4] = nan;
    err.clear();
    printf("refused: %s\n", capsule_ends_validate(a3.data(), b3.data(), nullptr, nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    a3[4] = -0.02; b3[5] = 0.03;   // (rod 1: b = a)
    err.clear();
    printf("refused: %s\n", capsule_ends_validate(a3.data(), b3.data(), nullptr, nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    b3[5] = 0.125; pb[8] = inf;
    err.clear();
    printf("refused: %s\n", capsule_ends_validate(a3.data(), b3.data(), pa.data(), pb.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    pb[8] = 0.25; pb[6] = -3.0;   // (rod 2: bp = ap)
    err.clear();
    printf("refused: %s\n", capsule_ends_validate(a3.data(), b3.data(), pa.data(), pb.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    pb[6] = -0.75;
    err.clear();
    printf("refused: %s\n", capsule_ends_validate(a3.data(), b3.data(), pa.data(), nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    err.clear();
    printf("refused: %s\n", capsule_ends_validate(a3.data(), b3.data(), nullptr, pb.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    if (capsule_ends_validate(a3.data(), b3.data(), pa.data(), pb.data(), S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("moved_a", a3); show("moved_b", b3); show("moved_ap", pa); show("moved_bp", pb);
    show("table_moved", table(S));
    if (capsule_ends_validate(a3.data(), b3.data(), nullptr, nullptr, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("table_at_rest", table(S));
  }
  // masks: the default, a given one, a bit at or above n
  std::vector<uint8_t> mask, mask0;
  if (shape_mask_validate("capsule", NV, 3, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_all", mask);
  mask0 = mask;
  std::vector<uint8_t> given(NV, 5); given[7] = 0; given[9] = 8;
  err.clear();
  printf("refused: %s\n", shape_mask_validate("capsule", NV, 3, given.data(), mask, err) ? err.c_str() : "NOT REFUSED");
  kept &= (mask == mask0);
  given[9] = 2;
  if (shape_mask_validate("capsule", NV, 3, given.data(), mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_given", mask);
  if (shape_mask_validate("capsule", NV, 8, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_eight", mask);
  // no capsules: valid, an empty table
  CapsuleTable E{};
  if (capsule_validate(nullptr, nullptr, nullptr, nullptr, 0, E, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  printf("empty: %d\n", E.n);
  printf("kept: %d\n", kept);
  printf("done\n");
  return 0;
}
