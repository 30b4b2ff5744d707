// Indexed parameter keys of tsl_set_param / tsl_param_grad_keys: "cloth<i>.<field>", "elastic<i>.<field>", "self_contact<b>", one parser for both
// entry points; and the keys tsl_param_grad_keys differentiates: their table, key -> (class, row) and the layout of the partial sums.  Plain C++
// (tests/test_ctx_tables.py drives it on the CPU through tests/native/tables_ref.cpp).
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

struct IndexedKey {
  enum Family { None, Cloth, Elastic, SelfContact } family;
  long index;
  std::string field;   // behind the first '.', empty for self_contact
};

// 0 with family == None: the key has none of the three prefixes in indexed form ("cloth" / "elastic" need a '.' somewhere behind them).
// -1: the prefix is there (family says which) and the index is malformed.  An index is a plain decimal number with nothing between its
// digits and the '.' (the end of the string for self_contact): no sign other than a minus, no blanks -- "cloth+1.Kl", "cloth 1.Kl",
// "cloth.Kl", "cloth0x.Kl" are not keys.  The range of the index is the caller's business, who knows the counts.
static int parse_indexed_key(const char* key, IndexedKey& out) {
  out = IndexedKey{IndexedKey::None, 0, std::string()};
  const std::string k(key);
  const size_t dot = k.find('.');
  size_t p0, end;
  if (k.rfind("self_contact", 0) == 0) { out.family = IndexedKey::SelfContact; p0 = 12; end = k.size(); }
  else if (k.rfind("cloth", 0) == 0 && dot != std::string::npos) { out.family = IndexedKey::Cloth; p0 = 5; end = dot; }
  else if (k.rfind("elastic", 0) == 0 && dot != std::string::npos) { out.family = IndexedKey::Elastic; p0 = 7; end = dot; }
  else return 0;
  const char c0 = k.c_str()[p0];
  char* endp = nullptr;
  out.index = strtol(k.c_str() + p0, &endp, 10);
  if (endp != k.c_str() + end || end == p0 || !(isdigit((unsigned char)c0) || c0 == '-')) return -1;
  if (out.family != IndexedKey::SelfContact) out.field = k.substr(dot + 1);
  return 0;
}

// the entry of a {field name, value} table that carries the name f, or null
template <class T, size_t N>
static const T* field_find(const std::pair<const char*, T> (&tab)[N], const std::string& f) {
  for (const auto& e : tab)
    if (f == e.first) return &e.second;
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ the differentiated keys (tsl_param_grad_keys)
// A key's value is the sum of one row of per-workgroup partials.  The rows belong to classes, one per element pass of csrc/k_param.hpp; the
// partials of the classes a call needs lie behind one another in the order of this enum.
enum PgClass { PG_FACE, PG_HINGE, PG_TET, PG_CONTACT, PG_STVK, PG_HANDLE, PG_NCLASS };
enum { PG_ROW_K_CONTACT, PG_ROW_MU_CLOTH_ELASTIC, PG_ROW_MU_CLOTH_CLOTH };   // the rows of PG_CONTACT
// One row per differentiated key: "cloth<i>.<name>" / "elastic<i>.<name>" (family Cloth / Elastic) or the plain <name> (family None).  The key
// reads row `row + per * i` of its class, `per` = rows of the class per cloth or body; a plain key reads `row`.
struct PgKey { IndexedKey::Family family; const char* name; PgClass cls; int row, per; };
static const PgKey pg_keys[] = {
    {IndexedKey::Cloth, "Kl", PG_FACE, 0, 2}, {IndexedKey::Cloth, "Ka", PG_FACE, 1, 2}, {IndexedKey::Cloth, "Kb", PG_HINGE, 0, 1},
    {IndexedKey::Cloth, "stvk_mu", PG_STVK, 0, 2}, {IndexedKey::Cloth, "stvk_lam", PG_STVK, 1, 2},
    {IndexedKey::Elastic, "mu", PG_TET, 0, 2}, {IndexedKey::Elastic, "lam", PG_TET, 1, 2},
    {IndexedKey::None, "k_contact", PG_CONTACT, PG_ROW_K_CONTACT, 0}, {IndexedKey::None, "mu_cloth_elastic", PG_CONTACT, PG_ROW_MU_CLOTH_ELASTIC, 0},
    {IndexedKey::None, "mu_cloth_cloth", PG_CONTACT, PG_ROW_MU_CLOTH_CLOTH, 0}, {IndexedKey::None, "k_handle", PG_HANDLE, 0, 0}};
struct PgRow { PgClass cls; int row; };

// "cloth<i>.Kl|Ka|..., elastic<i>.mu|lam, k_contact, ...": the table as the error message lists it
static std::string pg_supported_keys() {
  std::string s;
  IndexedKey::Family last = IndexedKey::None;
  for (const PgKey& e : pg_keys) {
    if (e.family != IndexedKey::None && e.family == last) s += '|';
    else s += std::string(s.empty() ? "" : ", ") + (e.family == IndexedKey::Cloth ? "cloth<i>." : e.family == IndexedKey::Elastic ? "elastic<i>." : "");
    s += e.name;
    last = e.family;
  }
  return s;
}

// key -> (class, row), or -1 with the message in err (it names the key)
static int pg_resolve_key(const char* key, int n_cloth, int n_el, PgRow& out, std::string& err) {
  IndexedKey ik;
  err = "tsl_param_grad_keys: ";
  if (parse_indexed_key(key, ik) && ik.family != IndexedKey::SelfContact) { err += std::string("bad index in ") + key; return -1; }
  for (const PgKey& e : pg_keys) {
    if (e.family != ik.family || (e.family == IndexedKey::None ? std::string(key) : ik.field) != e.name) continue;
    const bool cloth = e.family == IndexedKey::Cloth;
    const int n = cloth ? n_cloth : n_el;
    if (e.family != IndexedKey::None && (ik.index < 0 || ik.index >= n)) {
      err += std::string(cloth ? "bad cloth index in " : "bad elastic index in ") + key + " (" + std::to_string(n) + (cloth ? " cloths)" : " bodies)");
      return -1;
    }
    out = PgRow{e.cls, e.row + e.per * (int)ik.index};
    err.clear();
    return 0;
  }
  err += std::string(key) + " is not a differentiated key (supported: " + pg_supported_keys() + ")";
  return -1;
}

// The (offset, count) table of k_pg_final, PG_KEYS_PER_LAUNCH keys per launch
#define PG_KEYS_PER_LAUNCH 32
struct PgTable { int n; int off[PG_KEYS_PER_LAUNCH], cnt[PG_KEYS_PER_LAUNCH]; };

// Where the partials lie.  A class that some key needs holds nb[q] partials (the workgroups of its pass, 0 with no such element) for each of its
// rows -- `per` rows per cloth or body, or the plain keys' rows -- and a class no key needs holds none.  off[q]: its first partial; total: all of
// them; chunks: the keys' (offset, count) in the order of the call.  A key's row is the same whichever other keys of its class a call asks for.
struct PgLayout { size_t off[PG_NCLASS], total; std::vector<PgTable> chunks; };
static int pg_layout(int n_cloth, int n_el, const int nb[PG_NCLASS], const bool need[PG_NCLASS], const std::vector<PgRow>& keys, PgLayout& L, std::string& err) {
  int rows[PG_NCLASS] = {};
  for (const PgKey& e : pg_keys) rows[e.cls] = std::max(rows[e.cls], e.family == IndexedKey::None ? e.row + 1 : e.per * (e.family == IndexedKey::Cloth ? n_cloth : n_el));
  L.total = 0;
  for (int q = 0; q < PG_NCLASS; q++) { L.off[q] = L.total; if (need[q]) L.total += (size_t)rows[q] * nb[q]; }
  if (L.total > (size_t)INT32_MAX) { err = "tsl_param_grad_keys: too many partials"; return -1; }
  L.chunks.assign((keys.size() + PG_KEYS_PER_LAUNCH - 1) / PG_KEYS_PER_LAUNCH, PgTable{});
  for (size_t j = 0; j < keys.size(); j++) {
    PgTable& tab = L.chunks[j / PG_KEYS_PER_LAUNCH];
    const int q = keys[j].cls;
    tab.off[tab.n] = (int)(L.off[q] + (size_t)keys[j].row * nb[q]);
    tab.cnt[tab.n++] = nb[q];
  }
  return 0;
}
