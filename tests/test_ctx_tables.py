"""The host tables tsl_ctx_create uploads (thinshelllab_amd/csrc/scene_tables.hpp), the indexed-key parser and the differentiated keys of
tsl_param_grad_keys -- their table, key -> (class, row) and the layout of the partial sums (csrc/param_keys.hpp) -- on the CPU:
tests/native/tables_ref.cpp compiles the two headers into a shim, the scenes come from the product's cloth and body builders through
context.scene_desc (the struct the engine itself hands to the library), and every table is compared exactly with its restatement in
tests/scene_tables_numpy.py.  The properties the kernels rely on are asserted one by one as well, so that a failure names the table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from scene_tables_numpy import expected_tables

HERE = os.path.dirname(os.path.abspath(__file__))
DT = 5e-3
NP_TYPE = {"i": np.int32, "u": np.uint32, "d": np.float64, "l": np.int64}


@pytest.fixture(scope="module")
def shim():
    from thinshelllab_amd._lib import SceneDesc
    src = os.path.join(HERE, "native", "tables_ref.cpp")
    lib = os.path.join(HERE, "native", "libtablesref.so")
    csrc = os.path.join(HERE, "..", "thinshelllab_amd", "csrc")
    deps = [src, os.path.join(HERE, "..", "include", "tsl_hip.h")] + [os.path.join(csrc, f) for f in ("scene_tables.hpp", "param_keys.hpp", "direct_sym.hpp")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", lib])
    L = C.CDLL(lib)
    L.tables_names.restype = C.c_char_p
    L.tables_sizes.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    L.tables_copy.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
    L.parse_indexed_key_c.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    L.pg_resolve_key_c.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.pg_supported_keys_c.restype = C.c_char_p
    IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    L.pg_layout_c.argtypes = [C.c_int, C.c_int, IP, IP, IP, IP, C.c_int, LP, LP, IP, IP, IP, C.c_int, C.c_char_p, C.c_int]
    return L


def _cloth(N, M, offset=0):
    from thinshelllab_amd.engine.model_fold_offset import Cloth
    c = Cloth(N, DT, 0.01 * N, 0, 40.0, offset, False, M)
    c.init(0.0, 0.0, 0.0)
    return c


def _ball(offset):
    from thinshelllab_amd.engine.model_elastic_offset import Elastic
    e = Elastic(DT, 0.02, offset, 2, 2, 2, load=True)
    e.init(0.0, 0.0, 0.05)
    return e


def _scene_args(cloths=(), bodies=(), tot_NV=None):
    nv = tot_NV if tot_NV is not None else sum(c.NV for c in cloths) + sum(e.n_verts for e in bodies)
    return dict(tot_NV=nv, dt=DT, mass=np.ones(nv), gravity=np.zeros((nv, 3)), frozen=np.zeros(3 * nv, np.int32),
                cloths=[c._desc() for c in cloths], elastics=[e._desc() for e in bodies])


def _scenes():
    two = [_cloth(3, 2), None]
    two[1] = _cloth(2, 2, offset=two[0].NV)
    c22 = _cloth(2, 2)
    return {
        "cloth_1x1": _scene_args([_cloth(1, 1)]),              # 4 vertices, 2 faces, 1 hinge: one slice that is mostly padding
        "cloth_7x7": _scene_args([_cloth(7, 7)]),              # exactly 64 vertices: one full slice
        "cloth_7x8": _scene_args([_cloth(7, 8)]),              # 72 vertices: a second slice of 8 rows, the permutation crosses the slice boundary
        "two_cloths": _scene_args(two),                        # v_offset and face_start on counter_face, hinge and face numbering
        "cloth_and_ball": _scene_args([c22], [_ball(c22.NV)]),  # cloth / tet split of the gather lists, tet slots behind the hinge slots
        "ball_alone": _scene_args([], [_ball(0)]),             # n_cface == 0
        "one_vertex": _scene_args(tot_NV=1),                   # no element at all: the pad_col corner
    }


SCENES = ["cloth_1x1", "cloth_7x7", "cloth_7x8", "two_cloths", "cloth_and_ball", "ball_alone", "one_vertex"]


@pytest.fixture(scope="module")
def tables(shim):
    """name -> (scene arguments, tables of the library's header, tables of the restatement): built once, read by every test"""
    from thinshelllab_amd.context import scene_desc
    names = [x.split(":") for x in shim.tables_names().decode().strip(",").split(",")]
    out = {}
    for name, args in _scenes().items():
        d, keep = scene_desc(**args)
        sizes = (C.c_longlong * len(names))()
        err = C.create_string_buffer(256)
        assert shim.tables_sizes(C.byref(d), sizes, err, 256) == 0, err.value
        arrs = [np.zeros(max(int(n), 1), NP_TYPE[t])[:int(n)] for (_, t), n in zip(names, sizes)]
        ptrs = (C.c_void_p * len(names))(*[a.ctypes.data if a.size else None for a in arrs])
        assert shim.tables_copy(C.byref(d), ptrs) == 0
        got = {k: a for (k, _), a in zip(names, arrs)}
        for a in got.values():
            a.setflags(write=False)
        out[name] = (args, got, expected_tables(**args))
        del keep
    assert sorted(out) == sorted(SCENES)
    return out


def _counts(T):
    keys = ("n_cface", "n_hinge", "n_tet", "n_slices", "n_slots", "nnzb", "n_cgblk", "n_cgblk_cloth", "vg_hinge0", "vg_tet0", "vg_ns")
    return dict(zip(keys, T["counts"].tolist()))


@pytest.mark.parametrize("name", SCENES)
def test_every_table_equals_its_restatement(tables, name):
    _, got, want = tables[name]
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        if got[k].dtype == np.float64:
            assert np.array_equal(got[k], want[k]), k
        else:
            assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), k


def test_the_scenes_reach_the_edges_they_are_there_for(tables):
    n = {k: _counts(v[1]) for k, v in tables.items()}
    assert (n["cloth_1x1"]["n_cface"], n["cloth_1x1"]["n_hinge"], n["cloth_1x1"]["n_slices"]) == (2, 1, 1) and tables["cloth_1x1"][0]["tot_NV"] == 4
    assert tables["cloth_7x7"][0]["tot_NV"] == 64 and n["cloth_7x7"]["n_slices"] == 1
    assert tables["cloth_7x8"][0]["tot_NV"] == 72 and n["cloth_7x8"]["n_slices"] == 2
    perm = tables["cloth_7x8"][1]["perm"]
    assert (perm[:64] >= 64).any() and (perm[64:] < 64).any()      # rows change slice under the permutation by length
    assert tables["two_cloths"][1]["cloth_i"].reshape(-1, 4)[1].tolist() == [12, 8, 12, 9]      # face_start, NF, v_offset, NV of the second cloth
    assert n["cloth_and_ball"]["n_tet"] == 295 and 0 < n["cloth_and_ball"]["n_cgblk_cloth"] < n["cloth_and_ball"]["n_cgblk"]
    assert n["ball_alone"]["n_cface"] == 0 and n["ball_alone"]["n_cgblk_cloth"] == 0 and n["ball_alone"]["n_cgblk"] > 0
    assert n["one_vertex"]["n_slots"] == 64 and n["one_vertex"]["nnzb"] == 1 and n["one_vertex"]["n_cgblk"] == 0


_ROWS = {}


def _rows(T):
    """the rows of the pattern as lists (split once per scene: the tables live as long as the module)"""
    key = id(T["row_ptr"])
    if key not in _ROWS:
        _ROWS[key] = [T["row_idx"][a:b] for a, b in zip(T["row_ptr"][:-1], T["row_ptr"][1:])]
    return _ROWS[key]


def _lookup(T, vi, vj):
    """address of block (vi, vj) from the pattern alone: nine entries 64 apart behind slot (slice, k, lane)"""
    row = _rows(T)[vi].tolist()
    p = int(T["rowpos"][vi])
    return (int(T["slice_off"][p >> 6]) + 64 * row.index(vj)) * 9 + (p & 63)


@pytest.mark.parametrize("name", SCENES)
def test_pattern_properties(tables, name):
    args, T, _ = tables[name]
    NV, rows, perm, rowpos = args["tot_NV"], _rows(T), T["perm"], T["rowpos"]
    assert np.array_equal(rowpos[perm], np.arange(NV)) and np.array_equal(perm[rowpos], np.arange(NV))      # rowpos is the inverse of perm
    lens = np.array([len(rows[v]) for v in perm])
    assert (np.diff(lens) <= 0).all()                                                                          # row lengths do not increase along perm
    assert _counts(T)["nnzb"] == lens.sum() and all(v in rows[v] for v in range(NV))
    for p in range(NV):
        v, s, lane = int(perm[p]), p >> 6, p & 63
        assert T["slice_len"][s] >= len(rows[v])
        col = T["colidx"][T["slice_off"][s] + 64 * np.arange(T["slice_len"][s]) + lane]
        assert np.array_equal(col[:len(rows[v])], rowpos[rows[v]]), p          # real slots: position of the row's k-th neighbour
        assert (col[len(rows[v]):] != p).all(), p                              # padded slots: never the row itself (k_mask_matrix's frozen-diagonal rule)
        assert T["diag_perm"][p] == _lookup(T, v, v) == T["dblk"][v]


@pytest.mark.parametrize("name", SCENES)
def test_trans_round_trips_and_marks_the_padding(tables, name):
    args, T, _ = tables[name]
    rows, trans = _rows(T), T["trans"]
    real = np.zeros(len(trans), bool)
    for v in range(args["tot_NV"]):
        p = int(T["rowpos"][v])
        for k, w in enumerate(rows[v].tolist()):
            slot = int(T["slice_off"][p >> 6]) + 64 * k + (p & 63)
            real[slot] = True
            t = int(trans[slot])
            assert t == _lookup(T, w, v)
            t_slot = (t - t % 64) // 9 + t % 64          # address = 9 x (slot - lane) + lane
            assert int(trans[t_slot]) == _lookup(T, v, w) == slot * 9 - 8 * (p & 63)
    assert np.array_equal(trans == -1, ~real)


@pytest.mark.parametrize("name", SCENES)
def test_gather_lists_hold_every_element_entry_once_under_its_block(tables, name):
    _, T, _ = tables[name]
    n = _counts(T)
    base, ptr, ent = T["cg_base"], T["cg_ptr"], T["cg_ent"].astype(np.int64)
    assert len(base) == n["n_cgblk"] and len(ptr) == n["n_cgblk"] + 1 and ptr[0] == 0 and ptr[-1] == len(ent) and (np.diff(ptr) > 0).all()
    assert len(ent) == 9 * n["n_cface"] + 16 * n["n_hinge"] + 16 * n["n_tet"] and len(np.unique(ent)) == len(ent)      # every (element, pair) once
    is_tet = (ent >> 30) == 1
    blk_of = np.repeat(np.arange(n["n_cgblk"]), np.diff(ptr))
    assert not is_tet[blk_of < n["n_cgblk_cloth"]].any() and is_tet[blk_of >= n["n_cgblk_cloth"]].all()                # cloth blocks first, then tet blocks only
    assert (np.diff(base[:n["n_cgblk_cloth"]]) > 0).all() and (np.diff(base[n["n_cgblk_cloth"]:]) > 0).all()
    fpos = np.empty(n["n_cface"], np.int64); fpos[T["forder"]] = np.arange(n["n_cface"])
    f2v, hv, tv = T["f2v"].reshape(-1, 3), T["hv"].reshape(-1, 4), T["tv"].reshape(-1, 4)
    face_of_pos = T["forder"]
    for e, b in zip(ent.tolist(), blk_of.tolist()):
        el, pair = (e & 0x3FFFFFFF) >> 4, e & 15
        if e >> 31:
            vi, vj = hv[el, pair // 4], hv[el, pair % 4]
        elif e >> 30:
            vi, vj = tv[el, pair // 4], tv[el, pair % 4]
        else:
            assert pair < 9
            vi, vj = f2v[face_of_pos[el], pair // 3], f2v[face_of_pos[el], pair % 3]      # faces are addressed by processing index
        assert base[b] == _lookup(T, int(vi), int(vj)), (e, b)
    assert np.array_equal(np.sort(fpos), np.arange(n["n_cface"]))


@pytest.mark.parametrize("name", SCENES)
def test_vertex_lists_are_the_slots_of_each_vertex_ascending(tables, name):
    args, T, _ = tables[name]
    n = _counts(T)
    assert (n["vg_hinge0"], n["vg_tet0"], n["vg_ns"]) == (3 * n["n_cface"], 3 * n["n_cface"] + 4 * n["n_hinge"], 3 * n["n_cface"] + 4 * n["n_hinge"] + 4 * n["n_tet"])
    vert_of_slot = np.concatenate([T["f2v"], T["hv"], T["tv"]])          # slot -> the vertex it belongs to
    assert len(vert_of_slot) == n["vg_ns"] == len(T["vg_idx"]) and len(T["vg_ptr"]) == args["tot_NV"] + 1
    for v in range(args["tot_NV"]):
        mine = T["vg_idx"][T["vg_ptr"][v]:T["vg_ptr"][v + 1]]
        assert (np.diff(mine) > 0).all() and np.array_equal(mine, np.nonzero(vert_of_slot == v)[0]), v


# ------------------------------------------------------------------------------------------------ key grammar
FAMILY = {"none": 0, "cloth": 1, "elastic": 2, "self_contact": 3}


def _parse(shim, key):
    fam, idx, field = C.c_int(-1), C.c_longlong(-1), C.create_string_buffer(64)
    rc = shim.parse_indexed_key_c(key.encode(), C.byref(fam), C.byref(idx), field, 64)
    return rc, fam.value, idx.value, field.value.decode()


@pytest.mark.parametrize("key,want", [("cloth0.Kl", ("cloth", 0, "Kl")), ("cloth12.stvk_mu", ("cloth", 12, "stvk_mu")), ("elastic3.lam", ("elastic", 3, "lam")),
                                      ("self_contact2", ("self_contact", 2, "")), ("cloth-1.Kb", ("cloth", -1, "Kb"))])      # (the range check is the caller's)
def test_indexed_keys_accepted(shim, key, want):
    assert _parse(shim, key) == (0, FAMILY[want[0]], want[1], want[2])


@pytest.mark.parametrize("key", ["cloth+0.Kl", "cloth 0.Kl", "cloth.Kl", "cloth0x.Kl", "elastic1 .mu", "self_contact", "self_contact1x", "self_contact+1"])
def test_indexed_keys_rejected(shim, key):
    assert _parse(shim, key)[0] == -1


@pytest.mark.parametrize("key", ["k_contact", "clothing", "elastic"])
def test_keys_of_no_indexed_family(shim, key):
    rc, fam, _, _ = _parse(shim, key)
    assert (rc, fam) == (0, FAMILY["none"])


# ------------------------------------------------------------------------------------------------ differentiated keys (tsl_param_grad_keys)
PG = {"face": 0, "hinge": 1, "tet": 2, "contact": 3, "stvk": 4, "handle": 5}
# the table of csrc/param_keys.hpp restated: name -> (class, row among the rows of one cloth / body, rows per cloth / body), plain name -> (class, row)
CLOTH_FIELDS = {"Kl": ("face", 0, 2), "Ka": ("face", 1, 2), "Kb": ("hinge", 0, 1), "stvk_mu": ("stvk", 0, 2), "stvk_lam": ("stvk", 1, 2)}
ELASTIC_FIELDS = {"mu": ("tet", 0, 2), "lam": ("tet", 1, 2)}
PLAIN_KEYS = {"k_contact": ("contact", 0), "mu_cloth_elastic": ("contact", 1), "mu_cloth_cloth": ("contact", 2), "k_handle": ("handle", 0)}
SUPPORTED = "cloth<i>.Kl|Ka|Kb|stvk_mu|stvk_lam, elastic<i>.mu|lam, k_contact, mu_cloth_elastic, mu_cloth_cloth, k_handle"
N_CLOTH, N_EL = 2, 1          # the scene description of the key tests


def _supported(n_cloth, n_el):
    """key -> (class number, row) of every differentiated key of a scene with these counts"""
    want = {}
    for fam, n, fields in (("cloth", n_cloth, CLOTH_FIELDS), ("elastic", n_el, ELASTIC_FIELDS)):
        for i in range(n):
            for f, (cls, r, per) in fields.items():
                want[f"{fam}{i}.{f}"] = (PG[cls], r + per * i)
    want.update({k: (PG[cls], r) for k, (cls, r) in PLAIN_KEYS.items()})
    return want


def _class_rows(n_cloth, n_el):
    rows = [0] * len(PG)
    for cls, row in _supported(n_cloth, n_el).values():
        rows[cls] = max(rows[cls], row + 1)
    return rows


def _resolve(shim, key, n_cloth, n_el):
    cls, row, err = C.c_int(-7), C.c_int(-7), C.create_string_buffer(512)
    rc = shim.pg_resolve_key_c(key.encode(), n_cloth, n_el, C.byref(cls), C.byref(row), err, 512)
    return rc, cls.value, row.value, err.value.decode()


def _layout(shim, nb, need, keys, n_cloth=N_CLOTH, n_el=N_EL):
    """(offsets per class, total, [(offset, count) per key], chunk lengths), or the message of the failure"""
    n = len(keys)
    I = lambda a: (C.c_int * max(len(a), 1))(*a)
    off, total = (C.c_longlong * len(PG))(), C.c_longlong(-1)
    koff, kcnt, chunk_n, err = I([0] * n), I([0] * n), I([0] * 8), C.create_string_buffer(256)
    rc = shim.pg_layout_c(n_cloth, n_el, I(nb), I([int(x) for x in need]), I([k[0] for k in keys]), I([k[1] for k in keys]), n, off, C.byref(total), koff, kcnt, chunk_n, 8, err, 256)
    if rc < 0:
        return err.value.decode()
    return list(off), total.value, list(zip(koff[:n], kcnt[:n])), list(chunk_n[:rc])


def test_every_supported_key_resolves_to_its_class_and_row(shim):
    want = _supported(N_CLOTH, N_EL)
    assert len(want) == 5 * N_CLOTH + 2 * N_EL + 4
    for key, (cls, row) in want.items():
        assert _resolve(shim, key, N_CLOTH, N_EL) == (0, cls, row, ""), key
    assert len(set(want.values())) == len(want)          # no two keys share a row
    assert shim.pg_supported_keys_c().decode() == SUPPORTED


@pytest.mark.parametrize("key", ["no_such_key", "eps_contact", "damping", "cloth0.k_angle", "elastic0.mu", "cloth1.Kl", "cloth-1.Kb", "cg_tol", "cloth+0.Kl", "cloth 0.Kl"])
def test_bad_keys_fail_and_the_message_names_them(shim, key):
    """the keys of tests/test_gpu_param_grad.py::test_errors_name_the_key on its scene: one cloth, no body"""
    rc, _, _, err = _resolve(shim, key, 1, 0)
    assert rc == -1 and key in err and err.startswith("tsl_param_grad_keys: ")
    if key in ("no_such_key", "eps_contact", "damping", "cloth0.k_angle", "cg_tol"):
        assert err == f"tsl_param_grad_keys: {key} is not a differentiated key (supported: {SUPPORTED})"
    assert _resolve(shim, "cloth0.Kl", 1, 0)[:3] == (0, PG["face"], 0)


NB = [2, 1, 0, 3, 2, 1]          # workgroups per class; no tet at all


@pytest.mark.parametrize("need", [[q == k for q in range(6)] for k in range(6)] + [[True] * 6], ids=lambda n: "".join("01"[x] for x in n))
def test_layout_offsets_are_the_running_sum_over_the_needed_classes(shim, need):
    rows = _class_rows(N_CLOTH, N_EL)
    assert rows == [4, 2, 2, 3, 4, 1]
    keys = [v for v in _supported(N_CLOTH, N_EL).values() if need[v[0]]]
    off, total, per_key, chunks = _layout(shim, NB, need, keys)
    run = 0
    for q in range(6):
        assert off[q] == run, q
        run += rows[q] * NB[q] if need[q] else 0
    assert total == run and chunks == ([len(keys)] if keys else [])
    assert per_key == [(off[cls] + row * NB[cls], NB[cls]) for cls, row in keys]
    if need[PG["tet"]]:          # a class without workgroups holds no partials: its keys sum nothing, the class behind it starts where it does
        assert off[PG["tet"] + 1] == off[PG["tet"]] and all(c == 0 for (cls, _), (_, c) in zip(keys, per_key) if cls == PG["tet"])
    rows_seen = [(o, o + c) for o, c in per_key if c]
    assert all(0 <= a and b <= total for a, b in rows_seen) and len(set(rows_seen)) == len(rows_seen)          # inside the buffer, no two keys on one row


def test_layout_33_keys_make_two_chunks_with_each_key_where_it_is_alone(shim):
    sup = list(_supported(N_CLOTH, N_EL).values())
    rng = np.random.default_rng(3)
    for pool, need in ((sup, [True] * 6), ([v for v in sup if v[0] == PG["face"]], [q == PG["face"] for q in range(6)])):
        keys = [pool[i] for i in rng.integers(0, len(pool), 33)]
        _, total, per_key, chunks = _layout(shim, NB, need, keys)
        assert chunks == [32, 1]
        for k, got in zip(keys, per_key):
            _, total1, alone, chunks1 = _layout(shim, NB, need, [k])
            assert chunks1 == [1] and alone == [got] and total1 == total
    assert _layout(shim, NB, [True] * 6, sup[:1] * 32)[3] == [32] and _layout(shim, NB, [True] * 6, sup[:1] * 64)[3] == [32, 32]


def test_layout_fails_above_int32(shim):
    need = [True] + [False] * 5
    assert _layout(shim, [2 ** 29 - 1] + NB[1:], need, [(0, 0)])[1] == 4 * (2 ** 29 - 1)          # 2^31 - 4: the largest total these counts reach
    assert _layout(shim, [2 ** 29] + NB[1:], need, [(0, 0)]) == "tsl_param_grad_keys: too many partials"
