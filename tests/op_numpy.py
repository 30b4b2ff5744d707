"""The operator of the Krylov solvers restated with numpy (test infrastructure for test_op_numpy.py and test_gpu_operator_alone.py; float64 or long
double by argument): the SELL-64 layout of thinshelllab_amd/csrc/k_solver.hpp decoded into (row, column, 3 x 3 block) entries, the frozen-dof mask of
k_mask_matrix / k_contact_mask, the row -> (constraint, slot) lists of the matrix-free contact blocks, their diagonal, the block-Jacobi inverse, the
product, and one iteration of the two-kernel PCG.  Written from what each array MEANS (the header comments), not from the loops of the kernels -- except
wave_product, which follows sell_wave_product's split of a slice into waves and trips so that mistakes in that split can be planted and measured.

Everything is in the solver's row order (position p = rowpos[vertex]); vectors are (NV, 3) or flat 3 NV.

Layout: position p = 64 s + lane; block column k of slice s holds, for lane L, column id colidx[slice_off[s] + 64 k + L] and the nine values
vals[(slice_off[s] + 64 k) * 9 + 64 e + L], e = 3 r + c.  Slots behind the end of a row point at column 0 (column 1 for position 0) and hold zeros.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SELL_U = 4


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ SELL-64 <-> entries
def sell_slots(slice_off, slice_len, NV):
    """(p, k, slot, value base) of every slot of every real row, slice by slice, column by column"""
    P, K = [], []
    for s, ln in enumerate(np.asarray(slice_len).tolist()):
        lanes = np.arange(min(64, NV - 64 * s))
        P.append(np.tile(64 * s + lanes, ln)); K.append(np.repeat(np.arange(ln), len(lanes)))
    p = np.concatenate(P) if P else np.zeros(0, np.int64)
    k = np.concatenate(K) if K else np.zeros(0, np.int64)
    off = np.asarray(slice_off, np.int64)[p >> 6]
    return p, k, off + 64 * k + (p & 63), (off + 64 * k) * 9 + (p & 63)


def sell_decode(slice_off, slice_len, colidx, vals, NV, dt=np.float64):
    """entries (rows, cols, blocks (n, 3, 3), k) of every slot of every real row, padded slots included (they hold zeros)"""
    p, k, slot, base = sell_slots(slice_off, slice_len, NV)
    B = np.asarray(vals)[base[:, None] + 64 * np.arange(9)[None, :]].astype(dt).reshape(-1, 3, 3)
    return p, np.asarray(colidx, np.int64)[slot], B, k


def sell_encode(slice_off, slice_len, NV, rows, k, blocks):
    """the value array that holds blocks[i] in column k[i] of row rows[i], zeros elsewhere"""
    off = np.asarray(slice_off, np.int64)
    vals = np.zeros(9 * int(off[-1]), np.asarray(blocks).dtype)
    base = (off[rows >> 6] + 64 * k) * 9 + (rows & 63)
    vals[base[:, None] + 64 * np.arange(9)[None, :]] = np.asarray(blocks).reshape(-1, 9)
    return vals


def real_slots(rows, cols, k, row_len):
    """which decoded entries are blocks of the pattern (the first row_len[p] columns of row p), not padding"""
    return k < np.asarray(row_len)[rows]


def to_csr(rows, cols, blocks, NV):
    import scipy.sparse as sp
    r = (3 * rows[:, None, None] + np.arange(3)[None, :, None] + 0 * np.arange(3)[None, None, :]).ravel()
    c = (3 * cols[:, None, None] + 0 * np.arange(3)[None, :, None] + np.arange(3)[None, None, :]).ravel()
    return sp.coo_matrix((np.asarray(blocks, np.float64).ravel(), (r, c)), shape=(3 * NV, 3 * NV)).tocsr()


def product(entries, x, dt=np.float64, absolute=False):
    """y = H x (absolute: |H| |x|) over (rows, cols, blocks) entries, (NV, 3)"""
    rows, cols, B = entries[:3]
    x = np.asarray(x, dtype=dt).reshape(-1, 3)
    B = np.asarray(B, dtype=dt)
    if absolute:
        B, x = np.abs(B), np.abs(x)
    y = np.zeros_like(x)
    np.add.at(y, rows, np.einsum("nij,nj->ni", B, x[cols]))
    return y


# ------------------------------------------------------------------------------------------------ the frozen-dof mask
def mask_blocks(rows, cols, blocks, fz, mdt2):
    """k_mask_matrix: entry (r, c) of block (p, q) is zero where component r of p or component c of q is frozen; the diagonal entry of a frozen
    component holds m / dt^2.  fz: 3-bit mask per position"""
    fz = np.asarray(fz, np.int64)
    bit = (fz[:, None] >> np.arange(3)[None, :]) & 1                       # (NV, 3)
    out = np.array(blocks, copy=True)
    dead = (bit[rows][:, :, None] | bit[cols][:, None, :]).astype(bool)
    out[dead] = 0
    d = np.nonzero(rows == cols)[0]
    for r in range(3):
        sel = d[bit[rows[d], r] == 1]
        out[sel, r, r] = np.asarray(mdt2)[rows[sel]]
    return out


def mask_contact(H, idx, frozen):
    """k_contact_mask: entry (r, c) of the 12 x 12 block of a constraint is zero where dof r % 3 of vertex idx[r // 3] or the same of c is frozen"""
    f = np.asarray(frozen).reshape(-1, 3)[np.asarray(idx)].reshape(len(idx), 12).astype(bool)       # (nc, 12)
    out = np.array(H, copy=True)
    out[f[:, :, None] | f[:, None, :]] = 0
    return out


# ------------------------------------------------------------------------------------------------ matrix-free contact rows
def contact_csr(idx, rowpos, NV):
    """(ptr, ent, rows4): the entries (constraint << 2) | slot of every row, ascending within the row; rows4[e] = the four rows of the entry's constraint"""
    idx = np.asarray(idx, np.int64).reshape(-1, 4)
    r4 = np.asarray(rowpos, np.int64)[idx]                                 # (nc, 4)
    q = np.arange(4 * len(idx))
    row_of = r4.ravel()
    order = np.lexsort((q, row_of))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=NV))])
    return ptr, q[order], r4[q[order] >> 2]


def contact_entries(ptr, ent, rows4, Hm, dt=np.float64, limit=None):
    """(rows, cols, blocks) of the contact part; limit: only the first `limit` entries of every row (a planted mistake)"""
    ent = np.asarray(ent, np.int64)
    n = len(ent)
    row_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    keep = np.ones(n, bool) if limit is None else (np.arange(n) - np.asarray(ptr)[row_of]) < limit
    c, a = ent >> 2, ent & 3
    H = np.asarray(Hm, dtype=dt).reshape(-1, 4, 3, 4, 3)
    B = H[c, a].transpose(0, 2, 1, 3)                                      # (n, b, 3, 3)
    rows = np.repeat(row_of[keep], 4)
    return rows, np.asarray(rows4, np.int64)[keep].ravel(), B[keep].reshape(-1, 3, 3)


def contact_diag(ptr, ent, Hm, NV, dt=np.float64):
    """c_diag: per row the sum of the diagonal 3 x 3 sub-blocks of its entries; also the sum of their magnitudes and the number of entries"""
    ent = np.asarray(ent, np.int64)
    row_of = np.repeat(np.arange(NV), np.diff(ptr))
    H = np.asarray(Hm, dtype=dt).reshape(-1, 4, 3, 4, 3)
    D = H[ent >> 2, ent & 3, :, ent & 3, :]
    out = np.zeros((NV, 3, 3), dt); mag = np.zeros((NV, 3, 3), dt)
    np.add.at(out, row_of, D); np.add.at(mag, row_of, np.abs(D))
    return out, mag, np.diff(ptr)


def diag_blocks(rows, cols, blocks, NV):
    """the diagonal block of every row (the padded slots never point at their own row)"""
    d = rows == cols
    out = np.zeros((NV, 3, 3), np.asarray(blocks).dtype)
    out[rows[d]] = np.asarray(blocks)[d]
    return out


def dinv(D, cdiag=None, dt=np.float64):
    import mg_numpy as mg
    D = np.asarray(D, dtype=dt)
    return mg.block_inverse(D if cdiag is None else D + np.asarray(cdiag, dtype=dt), dt)


# ------------------------------------------------------------------------------------------------ the product as the waves of a slice form it
def wave_product(slice_off, slice_len, colidx, vals, NV, x, WPS=4, dt=np.float64, mut=None):
    """y = H x formed as sell_wave_product does: wave w of a slice takes the block columns w, w + WPS, ...; a wave with 1, 2, 3 or SELL_U + 1 columns takes
    them in one trip, any other number in trips of SELL_U, where a column past the end repeats the trip's first one with weight 0.
    mut: "repeat_weight" (those repeats count), "drop_wave" (wave 1 of every slice contributes nothing), "drop_last_slice" (no rows of a partial last slice)"""
    x = np.asarray(x, dtype=dt).reshape(-1, 3)
    y = np.zeros((NV, 3), dt)
    vals = np.asarray(vals); colidx = np.asarray(colidx, np.int64)
    nks = set()
    for s, ln in enumerate(np.asarray(slice_len).tolist()):
        nl = min(64, NV - 64 * s)
        if mut == "drop_last_slice" and nl < 64:
            continue
        lanes = np.arange(nl)
        off = int(slice_off[s])

        def column(kcol, weight):
            c = colidx[off + 64 * kcol + lanes]
            B = vals[((off + 64 * kcol) * 9 + lanes)[:, None] + 64 * np.arange(9)[None, :]].astype(dt).reshape(-1, 3, 3)
            return weight * np.einsum("nij,nj->ni", B, x[c])
        for w in range(WPS):
            nk = (ln - w + WPS - 1) // WPS
            if nk <= 0:
                continue
            nks.add(nk)
            if mut == "drop_wave" and w == 1:
                continue
            acc = np.zeros((nl, 3), dt)
            if nk in (1, 2, 3, SELL_U + 1):
                for u in range(nk):
                    acc += column(w + u * WPS, 1.0)
            else:
                for k0 in range(w, ln, SELL_U * WPS):
                    for u in range(SELL_U):
                        kcol = k0 + u * WPS
                        if kcol < ln:
                            acc += column(kcol, 1.0)
                        else:
                            acc += column(k0, 1.0 if mut == "repeat_weight" else 0.0)
            y[64 * s + lanes] += acc
    return y, nks


# ------------------------------------------------------------------------------------------------ one PCG iteration (K1 then K2 of k_solver.hpp)
def pcg_iteration(H, precond, st, dt=np.float64, slice_rows=64, block_rows=256, mut=None):
    """the state after iteration n + 1 from the state st after n >= 1 iterations: a dict of x, r, z, p, Ap (flat, solver order), rzh (2,), part_rz, part_rr,
    iters.  H: v -> H v, precond: r -> z, both on flat vectors in dt.  Iteration j (0-based) has parity j & 1: K1 reads rz_old from rzh[parity ^ 1], writes
    rzh[parity]; beta = rz / rz_old, p = z + beta p_old, Ap = H z + beta Ap_old; K2: alpha = rz / sum(part_pAp), x += alpha p, r -= alpha Ap, z = M^-1 r.
    mut: "beta_slot" (rz_old from the slot K1 writes), "stale_Ap" (st["Ap_prev"], the Ap of the iteration before, in the recurrence)"""
    f = lambda a: np.asarray(a, dtype=dt)
    parity = int(st["iters"]) & 1
    rzh = f(st["rzh"]).copy()
    rz, rr = f(st["part_rz"]).sum(), f(st["part_rr"]).sum()
    rz_old = rzh[parity if mut == "beta_slot" else parity ^ 1]
    beta = rz / rz_old
    p = f(st["z"]) + beta * f(st["p"])
    Ap = H(f(st["z"])) + beta * f(st["Ap_prev"] if mut == "stale_Ap" else st["Ap"])
    rzh[parity] = rz
    n = len(p) // 3
    seg = lambda v, m: np.add.reduceat(v.reshape(n, 3).sum(1), np.arange(0, n, m))
    part_pAp = seg(p * Ap, slice_rows)
    alpha = rz / part_pAp.sum()
    x = f(st["x"]) + alpha * p
    r = f(st["r"]) - alpha * Ap
    z = precond(r)
    return dict(x=x, r=r, z=z, p=p, Ap=Ap, rzh=rzh, part_pAp=part_pAp, part_rz=seg(r * z, block_rows), part_rr=seg(r * r, block_rows), iters=int(st["iters"]) + 1,
                rr_last=rr, rz_last=rz, beta=beta, alpha=alpha, Ap_prev=f(st["Ap"]))


def pcg_start(H, precond, b, dt=np.float64, slice_rows=64, block_rows=256):
    """the state after iteration 0 of a run from x = 0 (first = 1: beta = 0, p = z, Ap = H z written, rz_old not read)"""
    f = lambda a: np.asarray(a, dtype=dt)
    r = f(b).copy()
    z = precond(r)
    n = len(r) // 3
    seg = lambda v, m: np.add.reduceat(v.reshape(n, 3).sum(1), np.arange(0, n, m))
    rz, rr = seg(r * z, block_rows).sum(), seg(r * r, block_rows).sum()
    p = z.copy()
    Ap = H(z)
    part_pAp = seg(p * Ap, slice_rows)
    alpha = rz / part_pAp.sum()
    x = alpha * p
    r = r - alpha * Ap
    z = precond(r)
    rzh = np.zeros(2, dt); rzh[0] = rz
    return dict(x=x, r=r, z=z, p=p, Ap=Ap, rzh=rzh, part_pAp=part_pAp, part_rz=seg(r * z, block_rows), part_rr=seg(r * r, block_rows), iters=1, rr_last=rr, rz_last=rz,
                Ap_prev=np.zeros_like(Ap))


# ------------------------------------------------------------------------------------------------ the derived bound of a product, and the test inputs
def product_bound(slice_len, n_contact, absHx):
    """|y - y_ref|_i <= gamma(3 slice_len + 12 entries_i + 8) (|H||x|)_i: every static block column costs its row three operations on the longest path
    (a multiplication and two additions, as many for a masked repeat), every contact entry twelve (four 3-vectors), the joins of the waves, of the
    lanes' shares of a contact row and of the two parts at most eight more"""
    NV = len(absHx)
    ln = np.asarray(slice_len, np.float64)[np.arange(NV) >> 6]
    n = 3 * ln + 12 * np.asarray(n_contact, np.float64) + 8
    return (gamma(n)[:, None] * np.asarray(absHx, np.float64)).astype(np.float64)


def seeded_blocks(n, seed):
    """(n, 3, 3) values for an import: not symmetric, nowhere zero, magnitudes from 2^-20 to 2^20, so that every slot of the layout is distinguishable"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], (n, 3, 3)) * rng.uniform(1.0, 2.0, (n, 3, 3)) * 2.0 ** rng.integers(-20, 21, (n, 3, 3))


def seeded_vectors(NV, seed, units=()):
    """(3 NV, 8 + 3 len(units)) in the solver's order: eight vectors that are nowhere zero and large at positions 0 and 1 (where the padded slots point),
    then the unit vectors of the given positions"""
    rng = np.random.default_rng(seed)
    X = rng.choice([-1.0, 1.0], (NV, 3, 8)) * rng.uniform(0.5, 2.0, (NV, 3, 8)) * 2.0 ** rng.integers(-6, 7, (NV, 3, 8))
    X[:2] *= 2.0 ** 30
    E = np.zeros((NV, 3, 3 * len(units)))
    for j, p in enumerate(units):
        for a in range(3):
            E[p, a, 3 * j + a] = 1.0
    return np.concatenate([X, E], 2).reshape(3 * NV, -1)


def corner_ties(perm, rowpos, f2v, NV, n=70):
    """(verts, faces, bary): n ties from n distinct vertices onto the one face of the vertex at the last position of the solver's order (a corner of the
    grid): that row gets n contact entries (more than one wave), the tie vertices one each; five of them lie in the last slice too"""
    f2v = np.asarray(f2v).reshape(-1, 3)
    corner = int(perm[NV - 1])
    faces = np.nonzero((f2v == corner).any(1))[0]
    face = int(faces[0])
    tri = set(f2v[face].tolist())
    last = [int(v) for v in perm[64 * ((NV - 1) // 64):NV] if int(v) not in tri][:5]
    rest = [v for v in range(NV // 3, NV) if v not in tri and v not in last][:n - len(last)]
    verts = np.array(last + rest, np.int32)
    rng = np.random.default_rng(11)
    b = rng.uniform(0.2, 0.5, (n, 3))
    b /= b.sum(1, keepdims=True)
    return verts, np.full(n, face, np.int32), b
