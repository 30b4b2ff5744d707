// Test program (never part of libtsl_hip.so): the checks and the gather lists of csrc/handle_face_host.hpp on the pattern of a small grid, printed
// as "name: integers" lines for tests/test_surface_handle_numpy.py, which builds it with -fsanitize=address,undefined and compares the lists with
// a NumPy construction of the same rule.  The refused lists print "refused: <message>"; the program ends with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/handle_face_host.hpp"
#include "../../thinshelllab_amd/csrc/scene_tables.hpp"

static void show(const char* name, const std::vector<int>& a) {
  printf("%s:", name);
  for (int x : a) printf(" %d", x);
  printf("\n");
}

int main() {
  // a grid of 9 x 8 cells (90 vertices: two slices of the pattern), every cell cut along the same diagonal
  const int N = 9, M = 8, NV = (N + 1) * (M + 1);
  std::vector<int> faces;
  std::vector<std::vector<int>> cliques;
  for (int i = 0; i < N; i++)
    for (int j = 0; j < M; j++) {
      const int a = i * (M + 1) + j, b = a + 1, d = a + M + 1, c = d + 1;
      for (int v : {a, b, c, a, c, d}) faces.push_back(v);
      cliques.push_back({a, b, c});
      cliques.push_back({a, c, d});
    }
  const int NF = (int)faces.size() / 3;
  Pattern P;
  build_pattern(NV, cliques, P);
  printf("NV: %d\n", NV);
  show("faces", faces);

  // several handles on one face (17), a (1, 0, 0) corner, an edge point, two faces meeting in a vertex, a face of the second slice, out of order
  const std::vector<int32_t> hf = {17, 40, 17, 3, 17, 16, 141, 40, 0};
  const std::vector<double> hb = {0.2, 0.3, 0.5,  1.0, 0.0, 0.0,  0.6, 0.1, 0.3,  0.5, 0.5, 0.0,  1.0 / 3, 1.0 / 3, 1.0 / 3,
                                  0.0, 0.25, 0.75,  0.1, 0.8, 0.1,  0.0, 0.0, 1.0,  0.7, 0.2, 0.1};
  const std::vector<double> hw = {1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 1.0, 1.0};
  const int32_t n = (int32_t)hf.size();
  std::string err;
  if (handle_face_validate(NV, NF, faces.data(), hf.data(), hb.data(), hw.data(), n, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  FaceHandleLists L;
  if (handle_face_lists(P, faces.data(), hf.data(), n, L, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("handle_faces", std::vector<int>(hf.begin(), hf.end()));
  show("fv", L.fv); show("vl_v", L.vl_v); show("vl_ptr", L.vl_ptr); show("vl_ent", L.vl_ent);
  show("bl_addr", L.bl_addr); show("bl_ptr", L.bl_ptr); show("bl_ent", L.bl_ent);
  // n = 0 and weights == nullptr are valid
  if (handle_face_validate(NV, NF, faces.data(), nullptr, nullptr, nullptr, 0, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  if (handle_face_validate(NV, NF, faces.data(), hf.data(), hb.data(), nullptr, n, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }

  // the refused lists: one offender each, behind two valid handles
  struct Bad { int32_t face; double b[3]; double w; };
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const Bad bad[] = {{NF, {0.2, 0.3, 0.5}, 1.0}, {-1, {0.2, 0.3, 0.5}, 1.0}, {5, {-0.1, 0.6, 0.5}, 1.0}, {5, {nan, 0.5, 0.5}, 1.0}, {5, {1.2, 0.0, 0.0}, 1.0},
                     {5, {0.3, 0.3, 0.3}, 1.0}, {5, {0.2, 0.3, 0.5}, -1.0}, {5, {0.2, 0.3, 0.5}, inf}};
  for (const Bad& q : bad) {
    std::vector<int32_t> f = {17, 40, q.face};
    std::vector<double> b = {0.2, 0.3, 0.5, 1.0, 0.0, 0.0, q.b[0], q.b[1], q.b[2]};
    std::vector<double> w = {1.0, 1.0, q.w};
    err.clear();
    const int rc = handle_face_validate(NV, NF, faces.data(), f.data(), b.data(), w.data(), 3, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
  }
  {   // a face whose vertices have no common block: the pattern of the grid without that face's clique
    std::vector<int> tab = faces;
    tab[3 * 5 + 2] = NV - 1;   // face 5 now joins vertices that share no element
    const std::vector<int32_t> f = {17, 5};
    err.clear();
    const int rc = handle_face_lists(P, tab.data(), f.data(), 2, L, err);
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
  }
  printf("done\n");
  return 0;
}
