// Indexed parameter keys of tsl_set_param / tsl_param_grad_keys: "cloth<i>.<field>", "elastic<i>.<field>", "self_contact<b>".  Plain C++, one
// parser for both entry points (tests/test_ctx_tables.py drives it on the CPU through tests/native/tables_ref.cpp).
#pragma once
#include <cctype>
#include <cstdlib>
#include <string>
#include <utility>

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
