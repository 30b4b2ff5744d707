// Test program (never part of libtsl_hip.so): the checks and the gather lists of csrc/handle_host.hpp on the pattern of a small grid, for a face
// list (three corners per handle) and a vertex list (one), printed as "name: integers" lines for tests/test_surface_handle_numpy.py, which builds
// it with -fsanitize=address,undefined and compares the lists with a NumPy construction of the same rule.  The refused lists print
// "refused: <message>"; the program ends with "done" and exit status 0.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../thinshelllab_amd/csrc/handle_host.hpp"
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
  HandleLists L;
  const std::vector<int> fv = handle_face_corners(faces.data(), hf.data(), n);
  if (handle_lists(P, fv.data(), n, 3, L, err, hf.data())) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("handle_faces", std::vector<int>(hf.begin(), hf.end()));
  show("fv", fv); show("vl_v", L.vl_v); show("vl_ptr", L.vl_ptr); show("vl_ent", L.vl_ent);
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
    const int rc = handle_lists(P, handle_face_corners(tab.data(), f.data(), 2).data(), 2, 3, L, err, f.data());
    printf("refused: %s\n", rc ? err.c_str() : "NOT REFUSED");
  }

  // a vertex list: out of order, across both slices of the pattern, the first and the last vertex among them; one corner per handle
  const std::vector<int32_t> hv = {71, 3, 89, 64, 0, 40, 63, 17, 88, 5};
  const int32_t nv = (int32_t)hv.size();
  if (handle_validate(NV, hv.data(), nullptr, nv, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  HandleLists V;
  if (handle_lists(P, std::vector<int>(hv.begin(), hv.end()).data(), nv, 1, V, err)) { printf("unexpected: %s\n", err.c_str()); return 1; }
  show("handle_verts", std::vector<int>(hv.begin(), hv.end()));
  show("v_vl_v", V.vl_v); show("v_vl_ptr", V.vl_ptr); show("v_vl_ent", V.vl_ent);
  show("v_bl_addr", V.bl_addr); show("v_bl_ptr", V.bl_ptr); show("v_bl_ent", V.bl_ent);
  std::vector<int> diag;   // the pattern's diagonal addresses, what the scene tables keep as their diagonal-block table
  for (int v = 0; v < NV; v++) diag.push_back(P.lookup(v, v));
  show("diag", diag);
  {   // the vertex list's refusals
    const std::vector<int32_t> twice = {3, 7, 7}, out = {NV};
    const std::vector<double> w = {1.0, -1.0};
    err.clear(); printf("refused: %s\n", handle_validate(NV, twice.data(), nullptr, 3, err) ? err.c_str() : "NOT REFUSED");
    err.clear(); printf("refused: %s\n", handle_validate(NV, out.data(), nullptr, 1, err) ? err.c_str() : "NOT REFUSED");
    err.clear(); printf("refused: %s\n", handle_validate(NV, hv.data(), w.data(), 2, err) ? err.c_str() : "NOT REFUSED");
  }
  printf("done\n");
  return 0;
}
