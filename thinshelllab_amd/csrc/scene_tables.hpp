// Host tables of a scene (tsl_ctx_create uploads them): element lists in global ids, the SELL-64 block pattern, the block address of every
// element entry, the gather lists of k_cloth_gather and k_vertex_gather, the transposed-block table.  Plain C++ with no device code and no
// context: this is the single place the packed gather-entry format and the slot layout are produced (tests/test_ctx_tables.py pins them
// on the CPU through tests/native/tables_ref.cpp).
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tsl_hip.h"
#include "direct_sym.hpp"

// per-cloth constants read by the kernels (device copy)
struct ClothDev {
  int face_start, NF, v_offset, NV;
  double dx, mass, Kl, Ka, Kb, k_angle;
};
struct ElasticDev {
  int kind, cell_start, n_cells, v_offset, n_verts;
  double mu, lam, alpha;
};

struct Pattern {
  std::vector<std::vector<int>> rows;  // original order
  std::vector<int> perm, rowpos, slice_off, slice_len, colidx, diag_perm;
  long n_slots = 0;
  int n_slices = 0;
  int lookup(int vi, int vj) const {
    const auto& r = rows[vi];
    auto it = std::lower_bound(r.begin(), r.end(), vj);
    if (it == r.end() || *it != vj) return -1;
    const int k = (int)(it - r.begin());
    const int p = rowpos[vi], s = p >> 6, lane = p & 63;
    return (int)(((long)slice_off[s] + 64L * k) * 9 + lane);
  }
};

static void build_pattern(int NV, const std::vector<std::vector<int>>& cliques, Pattern& P) {
  P.rows.assign(NV, {});
  for (int i = 0; i < NV; i++) P.rows[i].push_back(i);
  for (const auto& c : cliques)
    for (int a : c)
      for (int b : c) P.rows[a].push_back(b);
  for (auto& r : P.rows) { std::sort(r.begin(), r.end()); r.erase(std::unique(r.begin(), r.end()), r.end()); }
  P.perm.resize(NV);
  for (int i = 0; i < NV; i++) P.perm[i] = i;
  std::stable_sort(P.perm.begin(), P.perm.end(), [&](int a, int b) { return P.rows[a].size() > P.rows[b].size(); });
  P.rowpos.resize(NV);
  for (int p = 0; p < NV; p++) P.rowpos[P.perm[p]] = p;
  P.n_slices = (NV + 63) / 64;
  P.slice_off.assign(P.n_slices + 1, 0);
  P.slice_len.assign(P.n_slices, 0);
  long off = 0;
  for (int s = 0; s < P.n_slices; s++) {
    int len = 0;
    for (int l = 0; l < 64 && s * 64 + l < NV; l++) len = std::max(len, (int)P.rows[P.perm[s * 64 + l]].size());
    P.slice_len[s] = len;
    P.slice_off[s] = (int)off;
    off += 64L * len;
  }
  P.slice_off[P.n_slices] = (int)off;
  P.n_slots = off;
  P.colidx.assign(off, 0);
  P.diag_perm.assign(NV, 0);
  for (int p = 0; p < NV; p++) {
    const int v = P.perm[p], s = p >> 6, lane = p & 63;
    const auto& r = P.rows[v];
    // padded slots (k >= row length) hold zero blocks; their column must not be the row itself, otherwise the
    // frozen-diagonal rule of k_mask_matrix would hit them
    const int pad_col = (p == 0) ? (NV > 1 ? 1 : 0) : 0;
    for (int k = 0; k < P.slice_len[s]; k++) P.colidx[P.slice_off[s] + 64 * k + lane] = (k < (int)r.size()) ? P.rowpos[r[k]] : pad_col;
    P.diag_perm[p] = P.lookup(v, v);
  }
}

struct SceneTables {
  std::vector<ClothDev> h_cloth;
  std::vector<ElasticDev> h_el;
  std::vector<DsGrid> grids;     // cloths that are full grids / the bodies as dense blocks (nested dissection of the direct solver)
  std::vector<DsBlock> blocks;
  int n_cface = 0, n_hinge = 0, n_tet = 0;
  std::vector<int> f2v, cf, cp, cid;      // per cloth face (global ids): vertices, counter_face, counter_point, cloth id
  std::vector<double> V, li;              // rest area, rest lengths
  std::vector<int> hinfo, hv;             // n_hinge x 8 (f1, l, f2, p4, p21, unused) and x 4 vertices, sorted by stencil class
  std::vector<int> forder;                // faces in the order the face kernels take them
  std::vector<int> tv, tel;               // 4 global vertices, elastic id
  std::vector<double> tB, tW;
  Pattern P;
  long nnzb = 0;
  std::vector<int> cfblk, hgblk, tetblk, dblk;   // block address of every element entry (9 / 16 / 16 per element) and of every diagonal block
  // k_cloth_gather: per matrix block (address cg_base) the entries cg_ent[cg_ptr[b], cg_ptr[b + 1]), each bit 31 = hinge, bit 30 = tet,
  // element << 4 | local vertex pair (faces by processing index); the first n_cgblk_cloth blocks belong to the cloth, the rest to the bodies
  std::vector<int> cg_base, cg_ptr;
  std::vector<unsigned> cg_ent;
  int n_cgblk = 0, n_cgblk_cloth = 0;
  // k_vertex_gather: staging slots 3 f + l of the faces, vg_hinge0 + 4 h + j of the hinges, vg_tet0 + 4 t + j of the tets; per vertex ascending
  std::vector<int> vg_ptr, vg_idx;
  int vg_hinge0 = 0, vg_tet0 = 0, vg_ns = 0;
  std::vector<int> trans;                 // slot of block (r, c) -> address of the transposed block (c, r); -1 on the padding of a slice
};

static int build_scene_tables(const tsl_scene_desc* d, SceneTables& T, std::string& err) {
  const int NV = d->tot_NV;
  std::vector<std::vector<int>> cliques;

  // ---- cloth tables (global ids)
  std::vector<int>&f2v = T.f2v, &cf = T.cf, &cp = T.cp, &cid = T.cid, &hinfo = T.hinfo, &hv = T.hv;
  std::vector<double>&V = T.V, &li = T.li;
  int face_start = 0;
  for (int ci = 0; ci < d->n_cloth; ci++) {
    const tsl_cloth_desc& cd = d->cloths[ci];
    ClothDev cdv{face_start, cd.NF, cd.v_offset, cd.NV, cd.dx, cd.mass, cd.Kl, cd.Ka, cd.Kb, cd.k_angle};
    T.h_cloth.push_back(cdv);
    if ((cd.N + 1) * (cd.M + 1) == cd.NV) T.grids.push_back(DsGrid{cd.v_offset, cd.N, cd.M});
    for (int i = 0; i < cd.NF; i++) {
      for (int k = 0; k < 3; k++) {
        f2v.push_back(cd.f2v_host[3 * i + k] + cd.v_offset);
        const int nb = cd.counter_face_host[3 * i + k];
        cf.push_back(nb < 0 ? -1 : nb + face_start);
        cp.push_back(cd.counter_point_host[3 * i + k]);
        li.push_back(cd.rest_len_host[3 * i + k]);
      }
      cid.push_back(ci);
      V.push_back(cd.rest_area_host[i]);
      cliques.push_back({cd.f2v_host[3 * i] + cd.v_offset, cd.f2v_host[3 * i + 1] + cd.v_offset, cd.f2v_host[3 * i + 2] + cd.v_offset});
    }
    for (int i = 0; i < cd.NF; i++)
      for (int l = 0; l < 3; l++) {
        const int nb = cd.counter_face_host[3 * i + l];
        if (nb > i) {
          const int p4 = cd.counter_point_host[3 * i + l];
          const int p11 = (l + 1) % 3;
          int p21 = (p4 + 1) % 3;
          if (cd.f2v_host[3 * i + p11] != cd.f2v_host[3 * nb + p21]) p21 = (p4 + 2) % 3;
          const int a = cd.f2v_host[3 * i + l] + cd.v_offset, b = cd.f2v_host[3 * i + (l + 1) % 3] + cd.v_offset;
          const int cc = cd.f2v_host[3 * i + (l + 2) % 3] + cd.v_offset, dd = cd.f2v_host[3 * nb + p4] + cd.v_offset;
          const int info[8] = {i + face_start, l, nb + face_start, p4, p21, 0, 0, 0};
          hinfo.insert(hinfo.end(), info, info + 8);
          hv.push_back(a); hv.push_back(b); hv.push_back(cc); hv.push_back(dd);
          cliques.push_back({a, b, cc, dd});
        }
      }
    face_start += cd.NF;
  }
  T.n_cface = face_start;
  T.n_hinge = (int)hv.size() / 4;
  {
    // Hinges sorted by stencil class (the offsets of their four vertices relative to the first), then by first vertex: the lanes of
    // a wave then add into CONSECUTIVE matrix rows (same block slot, neighbouring SELL lanes) -- 144 coalesced atomics per lane
    // instead of scattered ones.  Every hinge-indexed quantity is addressed through (face, edge), so the order is free.
    const int nh = T.n_hinge;
    std::map<std::array<int, 3>, int> cls;
    std::vector<int> key(nh), idx(nh);
    for (int h = 0; h < nh; h++) {
      const std::array<int, 3> t{hv[4 * h + 1] - hv[4 * h], hv[4 * h + 2] - hv[4 * h], hv[4 * h + 3] - hv[4 * h]};
      auto it = cls.find(t);
      if (it == cls.end()) it = cls.emplace(t, (int)cls.size()).first;
      key[h] = it->second; idx[h] = h;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return key[x] != key[y] ? key[x] < key[y] : hv[4 * x] < hv[4 * y]; });
    std::vector<int> hinfo2(hinfo.size()), hv2(hv.size());
    for (int h = 0; h < nh; h++) {
      std::copy(hinfo.begin() + 8 * (size_t)idx[h], hinfo.begin() + 8 * (size_t)idx[h] + 8, hinfo2.begin() + 8 * (size_t)h);
      std::copy(hv.begin() + 4 * (size_t)idx[h], hv.begin() + 4 * (size_t)idx[h] + 4, hv2.begin() + 4 * (size_t)h);
    }
    hinfo.swap(hinfo2); hv.swap(hv2);
  }

  // ---- tets
  std::vector<int>&tv = T.tv, &tel = T.tel;
  std::vector<double>&tB = T.tB, &tW = T.tW;
  int cell_start = 0;
  for (int ei = 0; ei < d->n_elastic; ei++) {
    const tsl_elastic_desc& ed = d->elastics[ei];
    ElasticDev edv{ed.kind, cell_start, ed.n_cells, ed.v_offset, ed.n_verts, ed.mu, ed.lam, ed.alpha};
    T.h_el.push_back(edv);
    T.blocks.push_back(DsBlock{ed.v_offset, ed.n_verts});
    for (int t = 0; t < ed.n_cells; t++) {
      std::vector<int> cl;
      for (int k = 0; k < 4; k++) { tv.push_back(ed.tets_host[4 * t + k] + ed.v_offset); cl.push_back(ed.tets_host[4 * t + k] + ed.v_offset); }
      tel.push_back(ei);
      for (int k = 0; k < 9; k++) tB.push_back(ed.B_host[9 * t + k]);
      tW.push_back(ed.W_host[t]);
      cliques.push_back(cl);
    }
    cell_start += ed.n_cells;
  }
  T.n_tet = cell_start;

  // ---- matrix pattern
  Pattern& P = T.P;
  build_pattern(NV, cliques, P);
  T.nnzb = 0;
  for (auto& r : P.rows) T.nnzb += (long)r.size();
  if (P.n_slots * 9 >= (1L << 31)) { err = "matrix too large for 32-bit slot offsets (" + std::to_string(P.n_slots) + " slots)"; return -1; }
  std::vector<int>&cfblk = T.cfblk, &hgblk = T.hgblk, &tetblk = T.tetblk, &dblk = T.dblk;
  cfblk.assign((size_t)T.n_cface * 9, 0); hgblk.assign((size_t)T.n_hinge * 16, 0); tetblk.assign((size_t)T.n_tet * 16, 0); dblk.assign(NV, 0);
  for (int f = 0; f < T.n_cface; f++)
    for (int l = 0; l < 3; l++)
      for (int m = 0; m < 3; m++) cfblk[(size_t)f * 9 + l * 3 + m] = P.lookup(f2v[3 * f + l], f2v[3 * f + m]);
  for (int h = 0; h < T.n_hinge; h++)
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 4; k++) hgblk[(size_t)h * 16 + j * 4 + k] = P.lookup(hv[4 * h + j], hv[4 * h + k]);
  for (int t = 0; t < T.n_tet; t++)
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 4; k++) tetblk[(size_t)t * 16 + j * 4 + k] = P.lookup(tv[4 * t + j], tv[4 * t + k]);
  for (int v = 0; v < NV; v++) dblk[v] = P.lookup(v, v);
  std::vector<int>& forder = T.forder;
  forder.assign(T.n_cface, 0);
  {
    std::map<std::array<int, 3>, int> cls;
    std::vector<int> key(T.n_cface);
    for (int f = 0; f < T.n_cface; f++) {
      const std::array<int, 3> t{f2v[3 * f + 1] - f2v[3 * f], f2v[3 * f + 2] - f2v[3 * f], 0};
      auto it = cls.find(t);
      if (it == cls.end()) it = cls.emplace(t, (int)cls.size()).first;
      key[f] = it->second; forder[f] = f;
    }
    std::stable_sort(forder.begin(), forder.end(), [&](int x, int y) { return key[x] != key[y] ? key[x] < key[y] : f2v[3 * x] < f2v[3 * y]; });
  }
  // gather assembly of the cloth Hessian (k_cloth_gather): per matrix block the list of (element, local vertex pair) that add to it
  std::vector<int>&cg_base = T.cg_base, &cg_ptr = T.cg_ptr;
  std::vector<unsigned>& cg_ent = T.cg_ent;
  {
    std::vector<std::pair<int, unsigned>> tup;
    tup.reserve((size_t)T.n_cface * 9 + (size_t)T.n_hinge * 16);
    std::vector<int> fpos(T.n_cface);   // face -> its processing index (the face kernel writes its record there)
    for (int t = 0; t < T.n_cface; t++) fpos[forder[t]] = t;
    for (int f = 0; f < T.n_cface; f++)
      for (int e = 0; e < 9; e++) tup.emplace_back(cfblk[(size_t)f * 9 + e], ((unsigned)fpos[f] << 4) | (unsigned)e);
    for (int h = 0; h < T.n_hinge; h++)
      for (int e = 0; e < 16; e++) tup.emplace_back(hgblk[(size_t)h * 16 + e], 0x80000000u | ((unsigned)h << 4) | (unsigned)e);
    for (int t = 0; t < T.n_tet; t++)   // the element blocks of the FEM bodies take the same road (bit 30)
      for (int e = 0; e < 16; e++) tup.emplace_back(tetblk[(size_t)t * 16 + e], 0x40000000u | ((unsigned)t << 4) | (unsigned)e);
    // blocks of the cloth first, blocks of the FEM bodies behind them (a block belongs to one kind: the two gathers run on different streams)
    auto is_tet = [](unsigned e) { return (e >> 30) == 1u; };
    std::sort(tup.begin(), tup.end(), [&](const std::pair<int, unsigned>& x, const std::pair<int, unsigned>& y) {
      if (is_tet(x.second) != is_tet(y.second)) return is_tet(y.second);
      return x < y;
    });
    cg_ent.reserve(tup.size());
    T.n_cgblk_cloth = 0;
    for (size_t i = 0; i < tup.size(); i++) {
      if (i == 0 || tup[i].first != tup[i - 1].first || is_tet(tup[i].second) != is_tet(tup[i - 1].second)) {
        cg_base.push_back(tup[i].first); cg_ptr.push_back((int)i);
        if (!is_tet(tup[i].second)) T.n_cgblk_cloth++;
      }
      cg_ent.push_back(tup[i].second);
    }
    cg_ptr.push_back((int)tup.size());
    T.n_cgblk = (int)cg_base.size();
    if (T.n_cface >= (1 << 26) || T.n_hinge >= (1 << 26) || T.n_tet >= (1 << 26)) { err = "mesh too large for the packed gather lists"; return -1; }
  }
  // vertex -> staging slots of the element gradients (k_vertex_gather): faces (3 f + l), hinges (+ 4 h + j), tets (+ 4 t + j), ascending
  std::vector<int>&vg_ptr = T.vg_ptr, &vg_idx = T.vg_idx;
  vg_ptr.assign(NV + 1, 0);
  {
    T.vg_hinge0 = 3 * T.n_cface; T.vg_tet0 = T.vg_hinge0 + 4 * T.n_hinge; T.vg_ns = T.vg_tet0 + 4 * T.n_tet;
    for (int v : f2v) vg_ptr[v + 1]++;
    for (int v : hv) vg_ptr[v + 1]++;
    for (int v : tv) vg_ptr[v + 1]++;
    for (int v = 0; v < NV; v++) vg_ptr[v + 1] += vg_ptr[v];
    vg_idx.resize(vg_ptr[NV]);
    std::vector<int> cur(vg_ptr.begin(), vg_ptr.end() - 1);
    for (size_t i = 0; i < f2v.size(); i++) vg_idx[cur[f2v[i]]++] = (int)i;
    for (size_t i = 0; i < hv.size(); i++) vg_idx[cur[hv[i]]++] = T.vg_hinge0 + (int)i;
    for (size_t i = 0; i < tv.size(); i++) vg_idx[cur[tv[i]]++] = T.vg_tet0 + (int)i;
  }
  {   // slot of block (r, c) -> address of the transposed block (c, r) (k_zfrozen_gather); -1 on the padding of a slice
    std::vector<int>& trans = T.trans;
    trans.assign((size_t)P.n_slots, -1);
    for (int v = 0; v < NV; v++) {
      const int pr = P.rowpos[v], sl = pr >> 6, lane = pr & 63;
      for (int k = 0; k < (int)P.rows[v].size(); k++) trans[(size_t)P.slice_off[sl] + 64 * (size_t)k + lane] = P.lookup(P.rows[v][k], v);
    }
  }
  return 0;
}
