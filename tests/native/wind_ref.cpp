// Test program (never part of libtsl_hip.so): the checks of csrc/wind_host.hpp and the gather lists a wind list gets from csrc/handle_host.hpp on
// the pattern of a grid of 2 x 2 cells, printed as "name: integers" lines for tests/test_wind_numpy.py, which builds it with
// -fsanitize=address,undefined and compares the lists with lists counted by hand.  The refused lists print "refused: <message>"; the program ends
// with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/handle_host.hpp"
#include "../../thinshelllab_amd/csrc/wind_host.hpp"

static void show(const char* name, const std::vector<int>& a) {
  printf("%s:", name);
  for (int x : a) printf(" %d", x);
  printf("\n");
}

int main() {
  // 2 x 2 cells, 9 vertices, every cell cut along the same diagonal: faces 0 .. 7 are the cloth's; faces 8, 9 stand for a body's surface
  const int N = 2, M = 2, NV = (N + 1) * (M + 1);
  std::vector<int> faces;
  std::vector<std::vector<int>> cliques;
  for (int i = 0; i < N; i++)
    for (int j = 0; j < M; j++) {
      const int a = i * (M + 1) + j, b = a + 1, d = a + M + 1, c = d + 1;
      for (int v : {a, b, c, a, c, d}) faces.push_back(v);
      cliques.push_back({a, b, c});
      cliques.push_back({a, c, d});
    }
  const int n_cface = (int)faces.size() / 3, NF = n_cface + 2;
  for (int v : {0, 1, 2, 3, 4, 5}) faces.push_back(v);
  Pattern P;
  build_pattern(NV, cliques, P);
  printf("NV: %d\n", NV);
  show("faces", faces);

  // three faces out of order: 6 and 3 share an edge, all three share vertex 4; one weight is zero
  const std::vector<int32_t> wf = {6, 0, 3};
  const std::vector<double> ww = {0.5, 0.0, 2.0};
  const int32_t n = (int32_t)wf.size();
  std::string err;
  if (wind_validate(n_cface, NF, wf.data(), ww.data(), n, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  if (wind_validate(n_cface, NF, wf.data(), nullptr, n, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  if (wind_validate(n_cface, NF, nullptr, nullptr, 0, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  const std::vector<int> cv = handle_face_corners(faces.data(), wf.data(), n);
  HandleLists L;
  if (handle_lists(P, cv.data(), n, 3, L, err, wf.data())) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("wind_faces", std::vector<int>(wf.begin(), wf.end()));
  show("cv", cv); show("vl_v", L.vl_v); show("vl_ptr", L.vl_ptr); show("vl_ent", L.vl_ent);
  show("bl_addr", L.bl_addr); show("bl_ptr", L.bl_ptr); show("bl_ent", L.bl_ent);
  std::vector<int> look;   // the pattern's address of every vertex pair (-1: no block)
  for (int a = 0; a < NV; a++)
    for (int b = 0; b < NV; b++) look.push_back(P.lookup(a, b));
  show("lookup", look);
  {   // every cloth face, in order
    std::vector<int32_t> all(n_cface);
    for (int f = 0; f < n_cface; f++) all[f] = f;
    if (wind_validate(n_cface, NF, all.data(), nullptr, n_cface, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
    HandleLists A;
    if (handle_lists(P, handle_face_corners(faces.data(), all.data(), n_cface).data(), n_cface, 3, A, err, all.data())) { printf("unexpected: %s\n", err.c_str()); return 1; }
    show("all_counts", std::vector<int>{(int)A.vl_v.size(), (int)A.vl_ent.size(), (int)A.bl_addr.size(), (int)A.bl_ent.size()});
  }

  // the refused lists: one offender each, behind two valid entries
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  struct Bad { int32_t face; double w; };
  const Bad bad[] = {{NF, 1.0}, {-1, 1.0}, {n_cface, 1.0}, {NF - 1, 1.0}, {6, 1.0}, {5, -0.25}, {5, nan}, {5, inf}};
  for (const Bad& q : bad) {
    const std::vector<int32_t> f = {3, 6, q.face};
    const std::vector<double> w = {1.0, 0.0, q.w};
    err.clear();
    printf("refused: %s\n", wind_validate(n_cface, NF, f.data(), w.data(), 3, err) ? err.c_str() : "NOT REFUSED");
  }
  err.clear();
  printf("refused: %s\n", wind_validate(n_cface, NF, wf.data(), nullptr, -2, err) ? err.c_str() : "NOT REFUSED");
  err.clear();
  printf("refused: %s\n", wind_validate(n_cface, NF, nullptr, nullptr, 2, err) ? err.c_str() : "NOT REFUSED");

  // the wind velocity: a refused one leaves the velocity in place
  double W[3] = {1.0, -2.0, 0.5};
  int kept = 1;
  const double w_nan[3] = {0.0, nan, 1.0}, w_inf[3] = {-inf, 0.0, 1.0}, w_ok[3] = {3.0, 0.0, -4.0};
  err.clear(); printf("refused: %s\n", wind_velocity_validate(w_nan, W, err) ? err.c_str() : "NOT REFUSED");
  kept &= (W[0] == 1.0 && W[1] == -2.0 && W[2] == 0.5);
  err.clear(); printf("refused: %s\n", wind_velocity_validate(w_inf, W, err) ? err.c_str() : "NOT REFUSED");
  kept &= (W[0] == 1.0 && W[1] == -2.0 && W[2] == 0.5);
  err.clear(); printf("refused: %s\n", wind_velocity_validate(nullptr, W, err) ? err.c_str() : "NOT REFUSED");
  kept &= (W[0] == 1.0 && W[1] == -2.0 && W[2] == 0.5);
  if (wind_velocity_validate(w_ok, W, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  printf("velocity: %g %g %g\n", W[0], W[1], W[2]);
  printf("kept: %d\n", kept);
  printf("done\n");
  return 0;
}
