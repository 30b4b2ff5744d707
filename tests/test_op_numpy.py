"""The restatement of the solvers' operator (op_numpy.py) pinned without the kernels: the SELL-64 decode against scipy's block CSR on the tables of
three scenes, the contact row lists on a hand-made constraint list, and planted mistakes -- each must exceed the derived product bound by decades on the
very inputs that tests/test_gpu_operator_alone.py feeds the kernels (seeded imported values, seeded vectors that are large where the padded slots point,
70 ties onto one corner face).  A mistake these inputs do not expose would mean the inputs are wrong."""
import numpy as np
import pytest
import scipy.sparse as sp

import cloth_numpy as cn
import op_numpy as op
from scene_tables_numpy import expected_tables

LD = np.longdouble


def _tables(args):
    T = expected_tables(**args)
    T["NV"] = int(args["tot_NV"])
    T["row_len"] = np.diff(T["row_ptr"])[T["perm"]]
    return T


def _encode(T, blocks):
    """SELL values of (nnzb, 3, 3) blocks in the order of (row_ptr, row_idx)"""
    row = np.repeat(np.arange(T["NV"]), np.diff(T["row_ptr"]))
    k = np.arange(len(row)) - T["row_ptr"][row]
    return op.sell_encode(T["slice_off"], T["slice_len"], T["NV"], T["rowpos"][row], k, blocks), row, k


def _drape(N, M):
    c = cn.ClothTables(N, M, 0.1 / 15)
    return dict(tot_NV=c.NV, cloths=[c.desc]), c


@pytest.fixture(scope="module")
def scenes():
    import test_ctx_tables as tct
    S = tct._scenes()
    out = {k: _tables(S[k]) for k in ("cloth_7x8", "cloth_and_ball", "cloth_1x1")}
    for N, M in ((8, 8), (12, 20)):
        args, c = _drape(N, M)
        out["drape_%dx%d" % (N, M)] = _tables(args)
        out["drape_%dx%d" % (N, M)]["f2v"] = np.asarray(c.desc["f2v"]).reshape(-1, 3)
    return out


@pytest.mark.parametrize("name", ["cloth_7x8", "cloth_and_ball", "cloth_1x1"])
def test_decode_of_encode_is_the_identity_and_the_product_is_scipys(scenes, name):
    T = scenes[name]
    NV, nnzb = T["NV"], len(T["row_idx"])
    B = op.seeded_blocks(nnzb, 1)
    vals, row, k = _encode(T, B)
    rows, cols, blocks, kk = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], vals, NV)
    real = op.real_slots(rows, cols, kk, T["row_len"])
    assert real.sum() == nnzb and not blocks[~real].any()
    # every real slot holds the block it was given, under the column it belongs to
    got = {(int(r), int(c)): b for r, c, b in zip(rows[real], cols[real], blocks[real])}
    for i in range(nnzb):
        assert np.array_equal(got[(int(T["rowpos"][row[i]]), int(T["rowpos"][T["row_idx"][i]]))], B[i])
    assert np.array_equal(op.sell_encode(T["slice_off"], T["slice_len"], NV, rows[real], kk[real], blocks[real]), vals)
    # padded slots point at column 0 (1 for position 0): never at their own row
    assert np.all(cols[~real] == np.where(rows[~real] == 0, min(1, NV - 1), 0))
    A = sp.bsr_matrix((B, T["row_idx"], T["row_ptr"]), shape=(3 * NV, 3 * NV))
    X = op.seeded_vectors(NV, 2, units=(0, NV - 1))
    for j in range(X.shape[1]):
        xo = np.zeros(3 * NV); xo.reshape(NV, 3)[T["perm"]] = X[:, j].reshape(NV, 3)        # caller's order
        ref = (A @ xo).reshape(NV, 3)[T["perm"]]
        y = op.product((rows, cols, blocks), X[:, j])
        scale = op.product((rows, cols, blocks), X[:, j], absolute=True)
        assert np.all(np.abs(y - ref) <= 64 * op.U * scale)
        yw, _ = op.wave_product(T["slice_off"], T["slice_len"], T["colidx"], vals, NV, X[:, j])
        assert np.all(np.abs(yw - ref) <= 64 * op.U * scale)
    assert abs(op.to_csr(rows, cols, blocks, NV) - op.to_csr(T["rowpos"][row], T["rowpos"][T["row_idx"]], B, NV)).max() == 0


def test_contact_rows_of_six_constraints_that_share_vertices():
    # vertices 0..6 in an order where rowpos is not the identity
    rowpos = np.array([3, 0, 6, 1, 5, 2, 4])
    idx = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [0, 1, 2, 5], [4, 3, 1, 0], [2, 5, 6, 0], [0, 1, 2, 6]])
    ptr, ent, rows4 = op.contact_csr(idx, rowpos, 7)
    # row of vertex v = rowpos[v]; its entries (constraint << 2 | slot) ascending
    by_vertex = {0: [0, 8, 15, 19, 20], 1: [1, 4, 9, 14, 21], 2: [2, 5, 10, 16, 22], 3: [3, 6, 13], 4: [7, 12], 5: [11, 17], 6: [18, 23]}
    for v, e in by_vertex.items():
        p = rowpos[v]
        assert ent[ptr[p]:ptr[p + 1]].tolist() == e, v
        for q in e:
            assert idx[q >> 2, q & 3] == v
    assert ptr[-1] == 24 and np.array_equal(rows4, rowpos[idx[ent >> 2]])
    # the product over the lists equals the sum of P_c^T H_c P_c
    rng = np.random.default_rng(0)
    H = rng.normal(size=(6, 12, 12))
    x = rng.normal(size=(7, 3))
    y = op.product(op.contact_entries(ptr, ent, rows4, H), x)
    ref = np.zeros((7, 3))
    for c in range(6):
        d = rowpos[idx[c]]
        ref[d] += (H[c] @ x[d].ravel()).reshape(4, 3)
    assert np.abs(y - ref).max() < 1e-13
    D, mag, cnt = op.contact_diag(ptr, ent, H, 7)
    assert cnt.tolist() == [len(by_vertex[v]) for v in np.argsort(rowpos)]
    for v, e in by_vertex.items():
        assert np.allclose(D[rowpos[v]], sum(H[q >> 2][3 * (q & 3):3 * (q & 3) + 3, 3 * (q & 3):3 * (q & 3) + 3] for q in e), atol=1e-14)
    frozen = np.zeros((7, 3), int); frozen[1, 2] = 1
    Hm = op.mask_contact(H, idx, frozen)
    for c in range(6):
        for a in range(4):
            dead = [3 * a + 2] if idx[c, a] == 1 else []
            for d in dead:
                assert not Hm[c, d].any() and not Hm[c, :, d].any()
    assert (Hm != 0).sum() == (H != 0).sum() - sum(2 * 12 - 1 for c in range(6) if 1 in idx[c])


def test_mask_rule_on_a_small_pattern():
    T = _tables(_drape(2, 1)[0])
    NV = T["NV"]
    vals, row, k = _encode(T, op.seeded_blocks(len(T["row_idx"]), 3))
    rows, cols, B, _ = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], vals, NV)
    fz = np.zeros(NV, np.uint8); fz[1] = 4; fz[2] = 3; fz[4] = 7
    md = np.arange(1.0, NV + 1)
    M = op.mask_blocks(rows, cols, B, fz, md)
    A, Am = op.to_csr(rows, cols, B, NV).toarray(), op.to_csr(rows, cols, M, NV).toarray()
    dead = np.zeros(3 * NV, bool)
    dead[[3 * 1 + 2, 3 * 2, 3 * 2 + 1, 3 * 4, 3 * 4 + 1, 3 * 4 + 2]] = True
    ref = A.copy()
    ref[dead] = 0; ref[:, dead] = 0
    for d in np.nonzero(dead)[0]:
        ref[d, d] = md[d // 3]
    assert np.array_equal(Am, ref)


# ------------------------------------------------------------------------------------------------ planted mistakes against the product bound
def _inputs(T, seed):
    NV = T["NV"]
    vals, _, _ = _encode(T, op.seeded_blocks(len(T["row_idx"]), seed))
    units = sorted({0, min(63, NV - 1), min(64, NV - 1), NV - 1})
    return vals, op.seeded_vectors(NV, seed + 1, units)


def _worst(T, vals, X, mutated, n_contact=None, extra=None):
    """largest |mutated - reference| / bound over the vectors"""
    NV = T["NV"]
    ent = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], vals, NV, LD)[:3]
    if extra is not None:
        ent = tuple(np.concatenate([a, b]) for a, b in zip(ent, extra))
    worst = 0.0
    for j in range(X.shape[1]):
        ref = op.product(ent, X[:, j], LD)
        bnd = op.product_bound(T["slice_len"], np.zeros(NV) if n_contact is None else n_contact, op.product(ent, X[:, j], LD, absolute=True))
        err = np.abs(mutated(X[:, j]).astype(LD) - ref).astype(np.float64)
        ok = bnd > 0
        worst = max(worst, float((err[ok] / bnd[ok]).max()))
        assert not np.any(err[~ok] > 0)
    return worst


@pytest.mark.parametrize("mut,name", [(None, "cloth_and_ball"), ("repeat_weight", "cloth_and_ball"), ("drop_wave", "drape_8x8"), ("drop_wave", "cloth_1x1"),
                                      ("drop_last_slice", "drape_8x8"), ("drop_last_slice", "drape_12x20")])
def test_planted_mistakes_in_the_wave_split_exceed_the_bound(scenes, mut, name):
    T = scenes[name]
    vals, X = _inputs(T, 7)
    wp = lambda x: op.wave_product(T["slice_off"], T["slice_len"], T["colidx"], vals, T["NV"], x, mut=mut)[0]
    w = _worst(T, vals, X, wp)
    print("operator restated, %s, %s: worst |y - ref| / bound %.3e" % (name, mut, w))
    if mut is None:
        nks = op.wave_product(T["slice_off"], T["slice_len"], T["colidx"], vals, T["NV"], X[:, 0])[1]
        assert 6 in nks            # a two-trip loop with masked repeats
        assert w <= 1.0
    else:
        assert w > 1e2


def test_contact_entries_behind_the_64th_dropped_exceed_the_bound(scenes):
    T = scenes["drape_12x20"]
    NV = T["NV"]
    vals, X = _inputs(T, 9)
    verts, faces, bary = op.corner_ties(T["perm"], T["rowpos"], T["f2v"], NV)
    idx = np.concatenate([T["f2v"][faces], verts[:, None]], 1)
    ptr, ent, rows4 = op.contact_csr(idx, T["rowpos"], NV)
    cnt = np.diff(ptr)
    last = np.arange(64 * ((NV - 1) // 64), NV)
    assert cnt[NV - 1] == 70 and np.any((cnt[last] >= 1) & (cnt[last] <= 63)) and np.any(cnt[last] == 0)
    # tie blocks: k w (b, -1) (b, -1)^T (x) I3
    H = np.zeros((70, 12, 12))
    for c in range(70):
        g = np.concatenate([bary[c], [-1.0]])
        H[c] = np.kron(1e3 * np.outer(g, g), np.eye(3))
    full = op.contact_entries(ptr, ent, rows4, H, LD)
    cut = op.contact_entries(ptr, ent, rows4, H, LD, limit=64)
    st = op.sell_decode(T["slice_off"], T["slice_len"], T["colidx"], vals, NV, LD)[:3]
    mutated = lambda x: op.product(tuple(np.concatenate([a, b]) for a, b in zip(st, cut)), x, LD)
    w = _worst(T, vals, X, mutated, cnt, full)
    print("operator restated, 12 x 20 with 70 ties: entries behind the 64th dropped: worst |y - ref| / bound %.3e" % w)
    assert w > 1e2
    good = lambda x: op.product(tuple(np.concatenate([a, b]) for a, b in zip(st, full)), x, np.float64)
    assert _worst(T, vals, X, good, cnt, full) <= 1.0


def _spd_system(T, seed):
    """a symmetric positive definite operator on the pattern of T and its block-Jacobi inverse"""
    NV = T["NV"]
    rng = np.random.default_rng(seed)
    A = sp.bsr_matrix((rng.normal(size=(len(T["row_idx"]), 3, 3)), T["row_idx"], T["row_ptr"]), shape=(3 * NV, 3 * NV)).toarray()
    A = A + A.T
    A += np.diag(np.abs(A).sum(1) * rng.uniform(1.001, 1.2, 3 * NV))
    P = np.repeat(3 * T["perm"], 3) + np.tile(np.arange(3), NV)
    A = A[P][:, P]
    Dinv = op.dinv(np.stack([A[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(NV)]))
    return A, Dinv, rng.normal(size=3 * NV)


@pytest.mark.parametrize("mut", ["stale_Ap", "beta_slot"])
def test_planted_mistakes_in_the_recurrence_exceed_the_bound(scenes, mut):
    import mg_numpy as mg
    T = scenes["drape_8x8"]
    A, Dinv, b = _spd_system(T, 4)
    H = lambda v: A.astype(v.dtype) @ v
    pre = lambda r: mg.block_apply(Dinv.astype(r.dtype), r)
    st = op.pcg_start(H, pre, b, LD)
    absA = np.abs(A)
    worst = np.inf
    for n in (1, 2, 3):
        nxt = op.pcg_iteration(H, pre, st, LD)
        if n >= 2:        # (the iteration behind the first has neither an Ap before the last one nor a second rz)
            bad = op.pcg_iteration(H, pre, st, LD, mut=mut)
            # the one-step bound on Ap (test_gpu_operator_alone.py): the product bound of H z plus three roundings of the recurrence
            bnd = op.gamma(3 * 13 + 10) * (absA @ np.abs(st["z"]).astype(np.float64)) + 3 * op.U * np.abs(float(nxt["beta"]) * st["Ap"]).astype(np.float64)
            r = float(np.max(np.abs(bad["Ap"] - nxt["Ap"]).astype(np.float64) / bnd))
            print("PCG restated, 8 x 8, %s at iteration %d: |Ap - ref| / bound %.3e" % (mut, n + 1, r))
            worst = min(worst, r)
        st = nxt
    assert worst > 1e2
    # and the restated iterations do solve the system
    for _ in range(120):
        st = op.pcg_iteration(H, pre, st, LD)
    assert np.linalg.norm((b - A @ st["x"].astype(np.float64))) <= 1e-10 * np.linalg.norm(b)
