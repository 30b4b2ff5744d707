// Test program (never part of libtsl_hip.so): the checks and the field table of csrc/sdf_host.hpp, printed as "name: numbers" lines for
// tests/test_sdf_numpy.py, which builds it with -fsanitize=address,undefined.  The refused lists print "refused: <message>"; the program ends
// with "done" and exit status 0.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/sdf_host.hpp"

template <class T>
static void show(const char* name, const std::vector<T>& a) {
  printf("%s:", name);
  for (T x : a) printf(" %.17g", (double)x);
  printf("\n");
}
static std::vector<double> table(const SdfTable& S) {
  std::vector<double> t;
  for (int j = 0; j < S.n; j++) t.insert(t.end(), S.row[j], S.row[j] + 30);
  return t;
}
static bool same(const SdfTable& A, const SdfTable& B) {
  return table(A) == table(B) && A.n == B.n && !memcmp(A.dim, B.dim, sizeof(A.dim)) && !memcmp(A.off, B.off, sizeof(A.off)) && A.smp == B.smp;
}

int main() {
  const int NV = 20;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string err;
  size_t total = 0;
  // a valid list of two fields: (4, 5, 6) with a quaternion that is not normalised, and (4, 4, 4)
  std::vector<double> smp(184);
  for (size_t e = 0; e < smp.size(); e++) smp[e] = 0.001 * (double)e - 0.05;
  const std::vector<int32_t> dims = {4, 5, 6, 4, 4, 4};
  const std::vector<double> O = {-0.01, -0.02, -0.03, 0.5, 0.25, -0.125}, H = {0.004, 0.01};
  const std::vector<double> C = {-0.02, 0.0, -0.005, 0.01, -0.02, 0.03};
  const std::vector<double> Q = {2.0, 0.2, -0.4, 0.6, 1.0, 0.0, 0.0, 0.0};
  const std::vector<double> off = {0.0005, -3.0}, mu = {0.0, 0.4};
  const double marker = 1.0;
  SdfTable S{};
  S.k = 7.0; S.eps = 0.5; S.eh = 0.25; S.smp = &marker;
  if (sdf_validate(smp.data(), dims.data(), O.data(), H.data(), C.data(), Q.data(), off.data(), mu.data(), 2, S, total, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("centres", C); show("quats", Q); show("origins", O); show("spacings", H); show("offsets", off); show("mu", mu);
  show("table", table(S));
  show("scalars", std::vector<double>{(double)S.n, S.k, S.eps, S.eh});
  show("dims", std::vector<double>{(double)S.dim[0][0], (double)S.dim[0][1], (double)S.dim[0][2], (double)S.dim[1][0], (double)S.dim[1][1], (double)S.dim[1][2]});
  show("offs", std::vector<double>{(double)S.off[0], (double)S.off[1]});
  show("total", std::vector<double>{(double)total});
  show("most", std::vector<double>{(double)SDF_SAMPLES_MAX});
  int kept = (S.smp == &marker);   // (the address of the buffer is the caller's)
  const SdfTable keep = S;

  // the refused lists: one offender each in field 1, behind a valid field 0 of (4, 4, 4); the list in place stays
  struct Bad { int32_t d[3]; double h, o[3], off, c[3], q[4], mu; int bad_sample; double bad_value; };
  const Bad ok = {{4, 4, 4}, 0.01, {0.0, 0.0, 0.0}, 0.0, {0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 0.0}, 0.1, -1, 0.0};
  std::vector<Bad> bad(15, ok);
  bad[0].d[1] = 3; bad[1].d[2] = 513;
  bad[2].h = 0.0; bad[3].h = -0.01; bad[4].h = nan; bad[5].h = inf;
  bad[6].o[1] = nan; bad[7].off = inf;
  bad[8].c[0] = nan;
  for (int a = 0; a < 4; a++) bad[9].q[a] = 0.0;
  bad[10].q[1] = nan;
  bad[11].mu = -0.5; bad[12].mu = nan;
  bad[13].bad_sample = 64 + (2 * 16 + 1 * 4 + 3); bad[13].bad_value = nan;
  bad[14].bad_sample = 0; bad[14].bad_value = -inf;
  for (const Bad& b : bad) {
    std::vector<double> s2(64 + 64 * 3, 0.25);   // (room for a third axis of 6 behind field 0; never more than 4 x 4 x 4 is read of field 1)
    if (b.bad_sample >= 0) s2[(size_t)b.bad_sample] = b.bad_value;
    const std::vector<int32_t> d2 = {4, 4, 4, b.d[0], b.d[1], b.d[2]};
    const std::vector<double> o2 = {0.0, 0.0, 0.0, b.o[0], b.o[1], b.o[2]}, h2 = {0.01, b.h}, f2 = {0.0, b.off};
    const std::vector<double> c2 = {0.0, 0.0, 1.0, b.c[0], b.c[1], b.c[2]}, q2 = {1.0, 0.0, 0.0, 0.0, b.q[0], b.q[1], b.q[2], b.q[3]}, m2 = {0.0, b.mu};
    err.clear();
    size_t t2 = 77;
    const int rc = sdf_validate(s2.data(), d2.data(), o2.data(), h2.data(), c2.data(), q2.data(), f2.data(), m2.data(), 2, S, t2, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
    kept &= (same(S, keep) && t2 == 77);
  }
  {   // nine fields; a negative count; a null list; more than 2^26 samples in total (refused on the dimensions: no sample is read)
    std::vector<double> s9(64 * 9, 0.5), o9(27, 0.0), h9(9, 0.01), c9(27, 1.0), q9(36, 0.5), f9(9, 0.0), m9(9, 0.0);
    std::vector<int32_t> d9(27, 4);
    err.clear();
    printf("refused: %s\n", sdf_validate(s9.data(), d9.data(), o9.data(), h9.data(), c9.data(), q9.data(), f9.data(), m9.data(), 9, S, total, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    err.clear();
    printf("refused: %s\n", sdf_validate(s9.data(), d9.data(), o9.data(), h9.data(), c9.data(), q9.data(), f9.data(), m9.data(), -1, S, total, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    err.clear();
    printf("refused: %s\n", sdf_validate(s9.data(), d9.data(), o9.data(), nullptr, c9.data(), q9.data(), f9.data(), m9.data(), 2, S, total, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    const std::vector<int32_t> dbig = {512, 512, 256, 512, 16, 16};
    err.clear();
    printf("refused: %s\n", sdf_validate(s9.data(), dbig.data(), o9.data(), h9.data(), c9.data(), q9.data(), f9.data(), m9.data(), 2, S, total, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    // eight are the most
    SdfTable S8{};
    if (sdf_validate(s9.data(), d9.data(), o9.data(), h9.data(), c9.data(), q9.data(), f9.data(), m9.data(), 8, S8, total, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    printf("eight: %d\n", S8.n);
    kept &= (total == 512 && S8.off[7] == 448);
  }
  // poses alone: a non-finite centre, a zero quaternion, a non-finite previous centre, a non-finite previous quaternion, one previous list without
  // the other; then all four given, then the previous ones left out
  {
    std::vector<double> c3 = C, q3 = Q, pc = C, pq = Q;
    c3[4] = nan;
    err.clear();
    printf("refused: %s\n", sdf_poses_validate(c3.data(), q3.data(), nullptr, nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    c3[4] = -0.02; q3[4] = 0.0;   // (field 1: a zero quaternion)
    err.clear();
    printf("refused: %s\n", sdf_poses_validate(c3.data(), q3.data(), nullptr, nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    q3[4] = 1.0; q3[5] = 1.0; c3[5] = 0.125; pc[5] = inf;
    err.clear();
    printf("refused: %s\n", sdf_poses_validate(c3.data(), q3.data(), pc.data(), pq.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    pc[5] = -0.75; pq[2] = nan;
    err.clear();
    printf("refused: %s\n", sdf_poses_validate(c3.data(), q3.data(), pc.data(), pq.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    pq[2] = -0.25;
    err.clear();
    printf("refused: %s\n", sdf_poses_validate(c3.data(), q3.data(), pc.data(), nullptr, S, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    err.clear();
    printf("refused: %s\n", sdf_poses_validate(c3.data(), q3.data(), nullptr, pq.data(), S, err) ? err.c_str() : "NOT REFUSED");
    kept &= same(S, keep);
    if (sdf_poses_validate(c3.data(), q3.data(), pc.data(), pq.data(), S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("moved_c", c3); show("moved_q", q3); show("moved_cp", pc); show("moved_qp", pq);
    show("table_moved", table(S));
    if (sdf_poses_validate(c3.data(), q3.data(), nullptr, nullptr, S, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("table_at_rest", table(S));
    kept &= (!memcmp(S.dim, keep.dim, sizeof(S.dim)) && !memcmp(S.off, keep.off, sizeof(S.off)) && S.smp == keep.smp);
  }
  // masks: a bit at or above n
  std::vector<uint8_t> mask, mask0;
  if (shape_mask_validate("field", NV, 2, nullptr, mask, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  mask0 = mask;
  std::vector<uint8_t> given(NV, 1); given[9] = 4;
  err.clear();
  printf("refused: %s\n", shape_mask_validate("field", NV, 2, given.data(), mask, err) ? err.c_str() : "NOT REFUSED");
  kept &= (mask == mask0);
  // no fields: valid, an empty table
  SdfTable E{};
  if (sdf_validate(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, E, total, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  printf("empty: %d\n", E.n);
  kept &= (total == 0);
  printf("kept: %d\n", kept);
  printf("done\n");
  return 0;
}
