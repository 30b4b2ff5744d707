// Test shim (never part of libtsl_hip.so): a flat C view of the host tables of a scene (csrc/scene_tables.hpp) and of the indexed-key parser
// and the differentiated keys' table, resolver and partial layout (csrc/param_keys.hpp), for tests/test_ctx_tables.py.  tables_names lists the arrays as "name:type," (i int32, u uint32, d double, l int64);
// tables_sizes builds the tables and reports the length of every array; tables_copy builds them again and copies every array out.
#include <cstring>

#include "../../thinshelllab_amd/csrc/param_keys.hpp"
#include "../../thinshelllab_amd/csrc/scene_tables.hpp"

namespace {
struct View { const char* name; char type; const void* p; size_t n; };
struct Flat {   // the members of SceneTables that are not plain arrays, flattened
  std::vector<int> cloth_i, el_i, grids, blocks, row_ptr, row_idx;
  std::vector<double> cloth_d, el_d;
  std::vector<long long> counts;
};
std::vector<View> views(const SceneTables& T, Flat& F) {
  for (const ClothDev& c : T.h_cloth) {
    for (int x : {c.face_start, c.NF, c.v_offset, c.NV}) F.cloth_i.push_back(x);
    for (double x : {c.dx, c.mass, c.Kl, c.Ka, c.Kb, c.k_angle}) F.cloth_d.push_back(x);
  }
  for (const ElasticDev& e : T.h_el) {
    for (int x : {e.kind, e.cell_start, e.n_cells, e.v_offset, e.n_verts}) F.el_i.push_back(x);
    for (double x : {e.mu, e.lam, e.alpha}) F.el_d.push_back(x);
  }
  for (const DsGrid& g : T.grids) for (int x : {g.v_offset, g.N, g.M}) F.grids.push_back(x);
  for (const DsBlock& b : T.blocks) for (int x : {b.v_offset, b.n_verts}) F.blocks.push_back(x);
  F.row_ptr.push_back(0);
  for (const auto& r : T.P.rows) { F.row_idx.insert(F.row_idx.end(), r.begin(), r.end()); F.row_ptr.push_back((int)F.row_idx.size()); }
  F.counts = {T.n_cface, T.n_hinge, T.n_tet, T.P.n_slices, T.P.n_slots, T.nnzb, T.n_cgblk, T.n_cgblk_cloth, T.vg_hinge0, T.vg_tet0, T.vg_ns};
  std::vector<View> v;
  auto I = [&](const char* n, const std::vector<int>& a) { v.push_back({n, 'i', a.data(), a.size()}); };
  auto D = [&](const char* n, const std::vector<double>& a) { v.push_back({n, 'd', a.data(), a.size()}); };
  v.push_back({"counts", 'l', F.counts.data(), F.counts.size()});
  I("cloth_i", F.cloth_i); D("cloth_d", F.cloth_d); I("el_i", F.el_i); D("el_d", F.el_d); I("grids", F.grids); I("blocks", F.blocks);
  I("f2v", T.f2v); I("cf", T.cf); I("cp", T.cp); I("cid", T.cid); D("V", T.V); D("li", T.li); I("hinfo", T.hinfo); I("hv", T.hv); I("forder", T.forder);
  I("tv", T.tv); I("tel", T.tel); D("tB", T.tB); D("tW", T.tW);
  I("row_ptr", F.row_ptr); I("row_idx", F.row_idx); I("perm", T.P.perm); I("rowpos", T.P.rowpos); I("slice_off", T.P.slice_off); I("slice_len", T.P.slice_len);
  I("colidx", T.P.colidx); I("diag_perm", T.P.diag_perm);
  I("cfblk", T.cfblk); I("hgblk", T.hgblk); I("tetblk", T.tetblk); I("dblk", T.dblk);
  I("cg_base", T.cg_base); I("cg_ptr", T.cg_ptr); v.push_back({"cg_ent", 'u', T.cg_ent.data(), T.cg_ent.size()});
  I("vg_ptr", T.vg_ptr); I("vg_idx", T.vg_idx); I("trans", T.trans);
  return v;
}
size_t width(char t) { return t == 'd' || t == 'l' ? 8 : 4; }
}  // namespace

extern "C" const char* tables_names(void) {
  static std::string s;
  if (s.empty()) {
    SceneTables T; Flat F;
    for (const View& w : views(T, F)) { s += w.name; s += ':'; s += w.type; s += ','; }
  }
  return s.c_str();
}

extern "C" int tables_sizes(const tsl_scene_desc* d, long long* sizes, char* err, int errlen) {
  SceneTables T; Flat F; std::string e;
  const int rc = build_scene_tables(d, T, e);
  if (err && errlen > 0) { strncpy(err, e.c_str(), errlen - 1); err[errlen - 1] = 0; }
  if (rc) return rc;
  int i = 0;
  for (const View& w : views(T, F)) sizes[i++] = (long long)w.n;
  return 0;
}

extern "C" int tables_copy(const tsl_scene_desc* d, void** dst) {
  SceneTables T; Flat F; std::string e;
  if (build_scene_tables(d, T, e)) return -1;
  int i = 0;
  for (const View& w : views(T, F)) { if (w.n) memcpy(dst[i], w.p, w.n * width(w.type)); i++; }
  return 0;
}

// parse_indexed_key as C: the return code, family as its enum value (None 0, Cloth 1, Elastic 2, SelfContact 3), index, field
extern "C" int parse_indexed_key_c(const char* key, int* family, long long* index, char* field, int fieldlen) {
  IndexedKey k;
  const int rc = parse_indexed_key(key, k);
  *family = (int)k.family; *index = k.index;
  if (field && fieldlen > 0) { strncpy(field, k.field.c_str(), fieldlen - 1); field[fieldlen - 1] = 0; }
  return rc;
}

// pg_resolve_key as C: the return code, (class, row), the message
extern "C" int pg_resolve_key_c(const char* key, int n_cloth, int n_el, int* cls, int* row, char* err, int errlen) {
  PgRow r{PG_NCLASS, -1};
  std::string e;
  const int rc = pg_resolve_key(key, n_cloth, n_el, r, e);
  *cls = (int)r.cls; *row = r.row;
  if (err && errlen > 0) { strncpy(err, e.c_str(), errlen - 1); err[errlen - 1] = 0; }
  return rc;
}

extern "C" const char* pg_supported_keys_c(void) {
  static const std::string s = pg_supported_keys();
  return s.c_str();
}

// pg_layout as C.  nb, need: PG_NCLASS entries each; the keys as (cls[j], row[j]), j < n_keys.  Out: off (PG_NCLASS entries), total, per key its
// (key_off[j], key_cnt[j]) read from the chunk tables, and the length of every chunk (chunk_n, at most max_chunks of them); returns the number of
// chunks, -1 on failure (message in err)
extern "C" int pg_layout_c(int n_cloth, int n_el, const int* nb, const int* need, const int* cls, const int* row, int n_keys, long long* off, long long* total,
                           int* key_off, int* key_cnt, int* chunk_n, int max_chunks, char* err, int errlen) {
  bool nd[PG_NCLASS];
  for (int q = 0; q < PG_NCLASS; q++) nd[q] = need[q] != 0;
  std::vector<PgRow> keys(n_keys);
  for (int j = 0; j < n_keys; j++) keys[j] = PgRow{(PgClass)cls[j], row[j]};
  PgLayout L;
  std::string e;
  const int rc = pg_layout(n_cloth, n_el, nb, nd, keys, L, e);
  if (err && errlen > 0) { strncpy(err, e.c_str(), errlen - 1); err[errlen - 1] = 0; }
  if (rc) return -1;
  for (int q = 0; q < PG_NCLASS; q++) off[q] = (long long)L.off[q];
  *total = (long long)L.total;
  int j = 0;
  for (size_t k = 0; k < L.chunks.size(); k++) {
    if ((int)k < max_chunks) chunk_n[k] = L.chunks[k].n;
    for (int i = 0; i < L.chunks[k].n; i++, j++) { key_off[j] = L.chunks[k].off[i]; key_cnt[j] = L.chunks[k].cnt[i]; }
  }
  return j == n_keys ? (int)L.chunks.size() : -1;
}
