"""The host tables of a scene (thinshelllab_amd/csrc/scene_tables.hpp) restated from their definitions with numpy set operations, stable
argsorts and dictionaries -- test infrastructure for tests/test_ctx_tables.py, written from what each table MEANS, not from the loops that
build it in the library.

Input: the keyword arguments of thinshelllab_amd.context.scene_desc (tot_NV, cloths, elastics).  Output: a dict of arrays under the names of
tests/native/tables_ref.cpp.

Definitions
  element lists   cloth faces, hinges and tets in global vertex ids, cloth after cloth, body after body.  A hinge is an interior edge, listed
                  at its face of lower index: (face i, edge l) with counter_face[i, l] > i, in (i, l) order; its vertices are the edge
                  (a, b), the third vertex c of face i and the vertex d of the other face opposite the edge.
  stencil class   of a hinge: (b - a, c - a, d - a); of a face: (v1 - v0, v2 - v0).  Classes are numbered in the order they first appear.
                  Hinges are STORED sorted by (class, a), faces are PROCESSED in the order sorted by (class, v0); ties keep list order.
  pattern         row v = {v} and every vertex that shares an element with v, ascending.  Rows sorted by falling length (ties by vertex)
                  give perm; 64 consecutive rows are a slice as wide as its longest row.  Slot k of the row at position p = 64 s + lane is
                  slice_off[s] + 64 k + lane; the address of block (v, w) is 9 x (slot - lane) + lane, lane = rowpos[v] & 63.
  padding         slots behind the end of a row hold column 0 -- column 1 for the row at position 0, so that no padded slot is a diagonal.
  gather lists    every (element, local vertex pair) as a packed entry under the address of its block: face entries (processing index << 4
                  | pair), hinge entries (bit 31 | h << 4 | pair), tet entries (bit 30 | t << 4 | pair).  Blocks of the cloth elements first,
                  ascending address, then blocks of the tets, ascending address; entries of a block ascending as unsigned numbers.
  vertex lists    staging slot 3 f + l belongs to vertex l of face f, 3 n_cface + 4 h + j to vertex j of hinge h, then 4 t + j of tet t behind
                  those; each vertex lists its slots ascending.
  trans           slot of block (v, w) -> address of block (w, v); -1 where a slot is padding.
"""
from collections import defaultdict

import numpy as np


def _first_appearance_ids(keys):
    seen = {}
    return np.array([seen.setdefault(tuple(k), len(seen)) for k in keys.tolist()], np.int64).reshape(-1)


def _by_class_then(keys, first):
    """indices sorted by (class of first appearance, first), ties in list order"""
    cls = _first_appearance_ids(keys)
    o = np.argsort(first, kind="stable")
    return o[np.argsort(cls[o], kind="stable")]


def expected_tables(*, tot_NV, cloths=(), elastics=(), **_):
    NV = int(tot_NV)
    i32 = lambda a, shape: np.asarray(a, np.int64).reshape(shape)
    out = {}
    # ---- element lists
    f2v, cf, cp, cid, V, li, hinfo, hv, cloth_i, cloth_d, grids = [], [], [], [], [], [], [], [], [], [], []
    fs = 0
    for ci, c in enumerate(cloths):
        F, nb_all, p_all, off = i32(c["f2v"], (-1, 3)), i32(c["counter_face"], (-1, 3)), i32(c["counter_point"], (-1, 3)), int(c["v_offset"])
        assert len(F) == c["NF"]
        cloth_i.append([fs, c["NF"], off, c["NV"]])
        cloth_d.append([c["dx"], c["mass"], c["Kl"], c["Ka"], c["Kb"], c["k_angle"]])
        if (c["N"] + 1) * (c["M"] + 1) == c["NV"]:
            grids.append([off, c["N"], c["M"]])
        f2v.append(F + off); cf.append(np.where(nb_all < 0, -1, nb_all + fs)); cp.append(p_all)
        cid.append(np.full(len(F), ci)); V.append(np.asarray(c["rest_area"], np.float64).reshape(-1)); li.append(np.asarray(c["rest_len"], np.float64).reshape(-1))
        i, l = np.nonzero(nb_all > np.arange(len(F))[:, None])     # row-major: (i, l) order
        nb, p4 = nb_all[i, l], p_all[i, l]
        b = F[i, (l + 1) % 3]
        p21 = np.where(F[nb, (p4 + 1) % 3] == b, (p4 + 1) % 3, (p4 + 2) % 3)
        hv.append(np.stack([F[i, l], b, F[i, (l + 2) % 3], F[nb, p4]], 1) + off)
        z = np.zeros_like(i)
        hinfo.append(np.stack([i + fs, l, nb + fs, p4, p21, z, z, z], 1))
        fs += len(F)
    cat = lambda parts, w, dt=np.int64: np.concatenate(parts).astype(dt).reshape(-1, w) if parts else np.zeros((0, w), dt)
    f2v, hv, hinfo = cat(f2v, 3), cat(hv, 4), cat(hinfo, 8)
    order = _by_class_then(hv[:, 1:] - hv[:, :1], hv[:, 0])
    hv, hinfo = hv[order], hinfo[order]
    forder = _by_class_then(f2v[:, 1:] - f2v[:, :1], f2v[:, 0])
    n_cface, n_hinge = len(f2v), len(hv)
    tv, tel, tB, tW, el_i, el_d, blocks = [], [], [], [], [], [], []
    cs = 0
    for ei, e in enumerate(elastics):
        Tt, off = i32(e["tets"], (-1, 4)), int(e["v_offset"])
        assert len(Tt) == e["n_cells"]
        el_i.append([e["kind"], cs, e["n_cells"], off, e["n_verts"]]); el_d.append([e["mu"], e["lam"], e["alpha"]]); blocks.append([off, e["n_verts"]])
        tv.append(Tt + off); tel.append(np.full(len(Tt), ei)); tB.append(np.asarray(e["B"], np.float64).reshape(-1)); tW.append(np.asarray(e["W"], np.float64).reshape(-1))
        cs += len(Tt)
    tv = cat(tv, 4)
    n_tet = len(tv)
    out.update(cloth_i=cat(cloth_i, 4), cloth_d=cat(cloth_d, 6, np.float64), el_i=cat(el_i, 5), el_d=cat(el_d, 3, np.float64), grids=cat(grids, 3), blocks=cat(blocks, 2),
               f2v=f2v, cf=cat(cf, 3), cp=cat(cp, 3), cid=cat(cid, 1), V=cat(V, 1, np.float64), li=cat(li, 1, np.float64), hinfo=hinfo, hv=hv, forder=forder,
               tv=tv, tel=cat(tel, 1), tB=cat(tB, 1, np.float64), tW=cat(tW, 1, np.float64))

    # ---- pattern: the set of (row, column) pairs
    def pairs_of(E):   # every ordered vertex pair of every element, element-major, local pair (j, k) -> j * width + k
        w = E.shape[1]
        return np.stack([np.repeat(E, w, axis=1).reshape(-1), np.tile(E, (1, w)).reshape(-1)], 1)
    elem_pairs = {"f": pairs_of(f2v), "h": pairs_of(hv), "t": pairs_of(tv)}
    diag = np.stack([np.arange(NV), np.arange(NV)], 1)
    P = np.unique(np.concatenate([diag] + list(elem_pairs.values())), axis=0)      # sorted by (row, column)
    rowlen = np.bincount(P[:, 0], minlength=NV)
    row_ptr = np.concatenate([[0], np.cumsum(rowlen)])
    perm = np.argsort(-rowlen, kind="stable")
    rowpos = np.empty(NV, np.int64); rowpos[perm] = np.arange(NV)
    n_slices = (NV + 63) // 64
    padded_len = np.zeros(n_slices * 64, np.int64); padded_len[:NV] = rowlen[perm]
    slice_len = padded_len.reshape(n_slices, 64).max(1) if n_slices else np.zeros(0, np.int64)
    slice_off = np.concatenate([[0], np.cumsum(64 * slice_len)])
    n_slots = int(slice_off[-1])
    k_of = np.arange(len(P)) - row_ptr[P[:, 0]]                                    # position of the pair in its row
    p_of = rowpos[P[:, 0]]
    slot = slice_off[p_of >> 6] + 64 * k_of + (p_of & 63)
    addr = (slot - (p_of & 63)) * 9 + (p_of & 63)
    address = {(int(r), int(c)): int(a) for (r, c), a in zip(P.tolist(), addr.tolist())}
    colidx = np.zeros(n_slots, np.int64)
    if NV > 1:
        colidx[0:slice_off[1]:64] = 1          # lane 0 of slice 0 is position 0: its padding points at column 1
    colidx[slot] = rowpos[P[:, 1]]
    trans = np.full(n_slots, -1, np.int64)
    trans[slot] = [address[(c, r)] for r, c in P.tolist()]
    look = lambda pr: np.array([address[tuple(x)] for x in pr.tolist()], np.int64)
    blk = {k: look(v) for k, v in elem_pairs.items()}
    out.update(row_ptr=row_ptr, row_idx=P[:, 1], perm=perm, rowpos=rowpos, slice_off=slice_off, slice_len=slice_len, colidx=colidx,
               diag_perm=look(np.stack([perm, perm], 1)), cfblk=blk["f"], hgblk=blk["h"], tetblk=blk["t"], dblk=look(diag), trans=trans)

    # ---- gather lists of the matrix blocks, from (block address, packed entry) pairs
    fpos = np.empty(n_cface, np.int64); fpos[forder] = np.arange(n_cface)
    ent_f = (np.repeat(fpos, 9) << 4) | np.tile(np.arange(9), n_cface)
    ent_h = (1 << 31) | (np.repeat(np.arange(n_hinge), 16) << 4) | np.tile(np.arange(16), n_hinge)
    ent_t = (1 << 30) | (np.repeat(np.arange(n_tet), 16) << 4) | np.tile(np.arange(16), n_tet)
    cloth_lists, tet_lists = defaultdict(list), defaultdict(list)
    for a, e in zip(np.concatenate([blk["f"], blk["h"]]).tolist(), np.concatenate([ent_f, ent_h]).tolist()):
        cloth_lists[a].append(e)
    for a, e in zip(blk["t"].tolist(), ent_t.tolist()):
        tet_lists[a].append(e)
    cg_base, cg_ptr, cg_ent = [], [0], []
    for lists in (cloth_lists, tet_lists):
        for a in sorted(lists):
            cg_base.append(a); cg_ent += sorted(lists[a]); cg_ptr.append(len(cg_ent))
    out.update(cg_base=np.array(cg_base, np.int64), cg_ptr=np.array(cg_ptr, np.int64), cg_ent=np.array(cg_ent, np.int64))

    # ---- staging slots of every vertex
    vert_of_slot = np.concatenate([f2v.reshape(-1), hv.reshape(-1), tv.reshape(-1)])
    out.update(vg_idx=np.argsort(vert_of_slot, kind="stable"), vg_ptr=np.concatenate([[0], np.cumsum(np.bincount(vert_of_slot, minlength=NV))]))
    out["counts"] = np.array([n_cface, n_hinge, n_tet, n_slices, n_slots, len(P), len(cg_base), len(cloth_lists), 3 * n_cface, 3 * n_cface + 4 * n_hinge,
                              3 * n_cface + 4 * n_hinge + 4 * n_tet], np.int64)
    return {k: np.asarray(v).reshape(-1) for k, v in out.items()}
