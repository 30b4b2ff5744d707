// Test program (never part of libtsl_hip.so): the checks and the slot records of csrc/tie_host.hpp on the face table of a small grid, and the place
// of the "k_tie" partials behind the table of csrc/param_keys.hpp, printed as "name: numbers" lines for tests/test_tie_numpy.py, which builds it
// with -fsanitize=address,undefined.  The refused lists print "refused: <message>"; the program ends with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/param_keys.hpp"
#include "../../thinshelllab_amd/csrc/tie_host.hpp"

template <class T>
static void show(const char* name, const std::vector<T>& a) {
  printf("%s:", name);
  for (T x : a) printf(" %.17g", (double)x);
  printf("\n");
}

int main() {
  // a grid of 9 x 8 cells (90 vertices), every cell cut along the same diagonal
  const int N = 9, M = 8, NV = (N + 1) * (M + 1);
  std::vector<int> faces;
  for (int i = 0; i < N; i++)
    for (int j = 0; j < M; j++) {
      const int a = i * (M + 1) + j, b = a + 1, d = a + M + 1, c = d + 1;
      for (int v : {a, b, c, a, c, d}) faces.push_back(v);
    }
  const int NF = (int)faces.size() / 3;
  printf("NV: %d\n", NV);
  show("faces", faces);

  // several ties per face (17) and per vertex (88), a one-hot stitch, an edge point, a weight 0, out of order
  const std::vector<int32_t> tv = {88, 89, 88, 70, 88, 3, 0, 45, 61};
  const std::vector<int32_t> tf = {17, 40, 17, 3, 16, 141, 100, 0, 17};
  const std::vector<double> tb = {0.2, 0.3, 0.5,  1.0, 0.0, 0.0,  0.6, 0.1, 0.3,  0.5, 0.5, 0.0,  1.0 / 3, 1.0 / 3, 1.0 / 3,
                                  0.0, 0.4, 0.6,  0.1, 0.8, 0.1,  0.0, 0.0, 1.0,  0.7, 0.2, 0.1};
  const std::vector<double> tw = {1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 1.0, 1.0};
  const int32_t n = (int32_t)tv.size();
  std::string err;
  if (tie_validate(NV, NF, faces.data(), tv.data(), tf.data(), tb.data(), tw.data(), n, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  const TieRecords R = tie_records(faces.data(), tv.data(), tf.data(), tb.data(), tw.data(), n);
  show("tie_verts", tv); show("tie_faces", tf); show("tie_bary", tb); show("tie_weights", tw);
  show("idx", R.idx); show("b", R.b); show("w", R.w);
  // n = 0 and weights == nullptr are valid; without weights every weight is 1
  if (tie_validate(NV, NF, faces.data(), nullptr, nullptr, nullptr, nullptr, 0, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  if (tie_validate(NV, NF, faces.data(), tv.data(), tf.data(), tb.data(), nullptr, n, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("w_default", tie_records(faces.data(), tv.data(), tf.data(), tb.data(), nullptr, n).w);
  show("idx_empty", tie_records(faces.data(), nullptr, nullptr, nullptr, nullptr, 0).idx);

  // the refused lists: one offender each, behind two valid ties
  struct Bad { int32_t vert, face; double b[3]; double w; };
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const Bad bad[] = {{88, NF, {0.2, 0.3, 0.5}, 1.0}, {88, -1, {0.2, 0.3, 0.5}, 1.0}, {NV, 5, {0.2, 0.3, 0.5}, 1.0}, {-1, 5, {0.2, 0.3, 0.5}, 1.0},
                     {faces[3 * 5 + 1], 5, {0.2, 0.3, 0.5}, 1.0}, {88, 5, {-0.1, 0.6, 0.5}, 1.0}, {88, 5, {nan, 0.5, 0.5}, 1.0}, {88, 5, {1.2, 0.0, 0.0}, 1.0},
                     {88, 5, {0.3, 0.3, 0.3}, 1.0}, {88, 5, {0.2, 0.3, 0.5}, -1.0}, {88, 5, {0.2, 0.3, 0.5}, inf}};
  for (const Bad& q : bad) {
    std::vector<int32_t> v = {88, 89, q.vert}, f = {17, 40, q.face};
    std::vector<double> b = {0.2, 0.3, 0.5, 1.0, 0.0, 0.0, q.b[0], q.b[1], q.b[2]};
    std::vector<double> w = {1.0, 1.0, q.w};
    err.clear();
    const int rc = tie_validate(NV, NF, faces.data(), v.data(), f.data(), b.data(), w.data(), 3, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
  }
  err.clear();
  printf("refused: %s\n", tie_validate(NV, NF, faces.data(), tv.data(), tf.data(), tb.data(), nullptr, -2, err) ? err.c_str() : "NOT REFUSED");

  // the "k_tie" partials lie behind the table's, whichever table keys are asked with it: for three sets of other keys (none; cloth0.Kl; every class)
  // the table's total without k_tie, then (offset, count, total) of k_tie with 2 workgroups, and the other keys' (offset, count) with k_tie asked too
  const int nb[PG_NCLASS] = {2, 1, 0, 3, 2, 1};
  const char* sets[3][3] = {{nullptr, nullptr, nullptr}, {"cloth0.Kl", nullptr, nullptr}, {"cloth1.Ka", "k_contact", "k_handle"}};
  for (int s = 0; s < 3; s++) {
    std::vector<PgRow> kr;
    bool need[PG_NCLASS] = {};
    for (int j = 0; j < 3 && sets[s][j]; j++) {
      PgRow r;
      if (pg_resolve_key(sets[s][j], 2, 1, r, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
      kr.push_back(r); need[r.cls] = true;
    }
    PgLayout L;
    if (pg_layout(2, 1, nb, need, kr, L, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    const PgTiePlace tp = pg_tie_place(L.total, 2);
    std::vector<long long> row = {(long long)L.total, (long long)tp.off, (long long)tp.cnt, (long long)tp.total};
    for (size_t j = 0; j < kr.size(); j++) { row.push_back(L.chunks[0].off[j]); row.push_back(L.chunks[0].cnt[j]); }
    char name[32];
    snprintf(name, sizeof(name), "place%d", s);
    show(name, row);
  }
  {   // no ties: no partials, the key sums nothing
    const PgTiePlace tp = pg_tie_place(7, 0);
    show("place_none", std::vector<long long>{(long long)tp.off, (long long)tp.cnt, (long long)tp.total});
  }
  {   // the table does not know the key: it is resolved ahead of it
    PgRow r;
    printf("table_knows_k_tie: %d\n", pg_resolve_key(PG_TIE_KEY, 2, 1, r, err) == 0 ? 1 : 0);
  }
  printf("done\n");
  return 0;
}
