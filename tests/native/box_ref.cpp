// Test program (never part of libtsl_hip.so): the checks and the box table of csrc/box_host.hpp, printed as "name: numbers" lines for
// tests/test_box_numpy.py, which builds it with -fsanitize=address,undefined.  The refused lists print "refused: <message>"; the program ends
// with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/box_host.hpp"

template <class T>
static void show(const char* name, const std::vector<T>& a) {
  printf("%s:", name);
  for (T x : a) printf(" %.17g", (double)x);
  printf("\n");
}
static std::vector<double> table(const BoxTable& S) {
  std::vector<double> t;
  for (int j = 0; j < S.n; j++) t.insert(t.end(), S.row[j], S.row[j] + 29);
  return t;
}

int main() {
  const int NV = 20;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string err;
  // a valid list of three boxes: a plate with a quaternion that is not normalised, a rod in all but name, a ball in all but name
  const std::vector<double> C = {-0.02, 0.0, -0.005,  0.01, -0.02, 0.03,  -3.0, 0.5, 0.25};
  const std::vector<double> Q = {2.0, 0.2, -0.4, 0.6,  1.0, 0.0, 0.0, 0.0,  -0.3, 0.5, 0.1, 0.8};
  const std::vector<double> H = {0.02, 0.015, 0.001,  0.04, 0.0, 0.0,  0.0, 0.0, 0.0};
  const std::vector<double> rad = {0.005, 0.002, 1.0e4}, mu = {0.0, 0.4, 1.5};
  BoxTable S{};
  S.k = 7.0; S.eps = 0.5; S.eh = 0.25;
  if (box_validate(C.data(), Q.data(), H.data(), rad.data(), mu.data(), 3, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("centres", C); show("quats", Q); show("half", H); show("radii", rad); show("mu", mu);
  show("table", table(S));
  show("scalars", std::vector<double>{(double)S.n, S.k, S.eps, S.eh});
  const std::vector<double> keep = table(S);

  // the refused lists: one offender each, behind a valid box; the list in place stays
  struct Bad { double c[3], q[4], h[3], r, mu; };
  const Bad bad[] = {{{nan, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, 0.1}, {{0.0, -inf, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {0.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, 0.1}, {{0.0, 0.0, 1.0}, {1.0, nan, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, inf, 0.0}, {1.0, 1.0, 1.0}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, -0.5, 1.0}, 0.1, 0.1}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, nan}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {inf, 1.0, 1.0}, 0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.0, 0.1}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, -0.1, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, nan, 0.1}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, inf, 0.1},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, -0.5}, {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, nan},
                     {{0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 0.1, inf}};
  int kept = 1;
  for (const Bad& b : bad) {
    const std::vector<double> c2 = {0.0, 0.0, 1.0, b.c[0], b.c[1], b.c[2]}, q2 = {1.0, 0.0, 0.0, 0.0, b.q[0], b.q[1], b.q[2], b.q[3]};
    const std::vector<double> h2 = {1.0, 0.0, 1.0, b.h[0], b.h[1], b.h[2]}, r2 = {1.0, b.r}, m2 = {0.0, b.mu};
    err.clear();
    const int rc = box_validate(c2.data(), q2.data(), h2.data(), r2.data(), m2.data(), 2, S, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
  }
  {   // nine boxes; a negative count; a null list
    std::vector<double> c9(27, 1.0), q9(36, 0.5), h9(27, 2.0), r9(9, 1.0), m9(9, 0.0);
    err.clear();
    printf("refused: %s\n", box_validate(c9.data(), q9.data(), h9.data(), r9.data(), m9.data(), 9, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    err.clear();
    printf("refused: %s\n", box_validate(c9.data(), q9.data(), h9.data(), r9.data(), m9.data(), -1, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    err.clear();
    printf("refused: %s\n", box_validate(c9.data(), nullptr, h9.data(), r9.data(), m9.data(), 2, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep && S.n == 3);
    // eight are the most
    BoxTable S8{};
    if (box_validate(c9.data(), q9.data(), h9.data(), r9.data(), m9.data(), 8, S8, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    printf("eight: %d\n", S8.n);
  }
  // poses alone: a non-finite centre, a zero quaternion, a non-finite previous centre, a non-finite previous quaternion, one previous list without
  // the other; then all four given, then the previous ones left out
  {
    std::vector<double> c3 = C, q3 = Q, pc = C, pq = Q;
    c3[4] = nan;
    err.clear();
    printf("refused: %s\n", box_poses_validate(c3.data(), q3.data(), nullptr, nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    c3[4] = -0.02; q3[4] = 0.0;   // (box 1: a zero quaternion)
    err.clear();
    printf("refused: %s\n", box_poses_validate(c3.data(), q3.data(), nullptr, nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    q3[4] = 1.0; q3[5] = 1.0; c3[5] = 0.125; pc[8] = inf;
    err.clear();
    printf("refused: %s\n", box_poses_validate(c3.data(), q3.data(), pc.data(), pq.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    pc[8] = -0.75; pq[2] = nan;
    err.clear();
    printf("refused: %s\n", box_poses_validate(c3.data(), q3.data(), pc.data(), pq.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    pq[2] = -0.25;
    err.clear();
    printf("refused: %s\n", box_poses_validate(c3.data(), q3.data(), pc.data(), nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    err.clear();
    printf("refused: %s\n", box_poses_validate(c3.data(), q3.data(), nullptr, pq.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= (table(S) == keep);
    if (box_poses_validate(c3.data(), q3.data(), pc.data(), pq.data(), S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("moved_c", c3); show("moved_q", q3); show("moved_cp", pc); show("moved_qp", pq);
    show("table_moved", table(S));
    if (box_poses_validate(c3.data(), q3.data(), nullptr, nullptr, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("table_at_rest", table(S));
  }
  // masks: the default, a given one, a bit at or above n
  std::vector<uint8_t> mask, mask0;
  if (shape_mask_validate("box", NV, 3, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_all", mask);
  mask0 = mask;
  std::vector<uint8_t> given(NV, 5); given[7] = 0; given[9] = 8;
  err.clear();
  printf("refused: %s\n", shape_mask_validate("box", NV, 3, given.data(), mask, err) ? err.c_str() : "NOT REFUSED");
  kept &= (mask == mask0);
  given[9] = 2;
  if (shape_mask_validate("box", NV, 3, given.data(), mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("mask_given", mask);
  // no boxes: valid, an empty table
  BoxTable E{};
  if (box_validate(nullptr, nullptr, nullptr, nullptr, nullptr, 0, E, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  printf("empty: %d\n", E.n);
  printf("kept: %d\n", kept);
  printf("done\n");
  return 0;
}
