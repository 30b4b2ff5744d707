"""NumPy restatement of soft handles at barycentric points of faces (csrc/k_handle.hpp): handle i sits on the face with the
vertices fv[i] = (v_0, v_1, v_2), has barycentric coordinates b[i] and ties the point p_i = sum_a b_a x_{v_a} to a world-space target t_i,

    E_h = 1/2 k sum_i w_i |p_i - t_i|^2,   H = k sum_i w_i (b_i b_i^T) (x) I_3 on the dofs of the face.

Dense: x is (NV, 3), the matrix (3 NV, 3 NV).  Frozen rule (the engine's mask rule): a frozen dof has no gradient entry, no matrix row or column of
the term, and contributes to no gradient with respect to a target or to k.  The energy, the points and the force read-out are not masked.
gather_lists restates the two gather lists of csrc/handle_host.hpp, block addresses included."""
import numpy as np


def _free(frozen, NV):
    return np.ones((NV, 3), bool) if frozen is None else ~np.asarray(frozen).reshape(NV, 3).astype(bool)


def points(x, fv, b):
    return np.einsum("ia,iac->ic", b, x[fv])


def energy(x, fv, b, w, t, k):
    d = points(x, fv, b) - t
    return 0.5 * k * float((w * (d * d).sum(1)).sum())


def gradient(x, fv, b, w, t, k, frozen=None):
    """(NV, 3): row v_a += k w_i b_a (p_i - t_i), zero on frozen dofs"""
    g = np.zeros_like(x)
    r = points(x, fv, b) - t
    for a in range(3):
        np.add.at(g, fv[:, a], (k * w * b[:, a])[:, None] * r)
    return g * _free(frozen, len(x))


def matrix(NV, fv, b, w, k, frozen=None):
    """(3 NV, 3 NV): k sum_i w_i (b_i b_i^T) (x) I_3, frozen rows and columns zero"""
    B = np.zeros((NV, NV))
    for a in range(3):
        for c in range(3):
            np.add.at(B, (fv[:, a], fv[:, c]), (k * w) * (b[:, a] * b[:, c]))
    H = np.kron(B, np.eye(3))
    m = _free(frozen, NV).ravel().astype(float)
    return H * m[:, None] * m[None, :]


def touched(NV, fv):
    """(3 NV, 3 NV) bool: the dofs pairs inside the touched blocks (v_a, v_b)"""
    B = np.zeros((NV, NV), bool)
    for a in range(3):
        for c in range(3):
            B[fv[:, a], fv[:, c]] = True
    return np.kron(B, np.ones((3, 3), bool))


def force(x, fv, b, w, t, k):
    """(n, 3): k w_i (t_i - p_i), the force the handle applies to the surface; not masked"""
    return k * w[:, None] * (t - points(x, fv, b))


def target_grad(p, fv, b, w, k, frozen=None):
    """(n, 3): -p . dF/dt_i, component c = k w_i sum_a b_a p_{v_a, c} over the corners whose dof (v_a, c) is free (F the masked gradient)"""
    p = p.reshape(-1, 3)
    pm = p * _free(frozen, len(p))
    return k * w[:, None] * np.einsum("ia,iac->ic", b, pm[fv])


def k_deriv(x, p, fv, b, w, t, frozen=None):
    """-p . dF/dk over the free dofs = -sum_i w_i sum_a b_a sum_{c free} p_{v_a, c} (p_i - t_i)_c"""
    p = p.reshape(-1, 3)
    pm = p * _free(frozen, len(x))
    r = points(x, fv, b) - t
    return -float((w[:, None] * np.einsum("ia,iac->ic", b, pm[fv]) * r).sum())


def block_addresses(NV, cliques):
    """{(row vertex, column vertex): block address} of the SELL-64 pattern built from the cliques (Pattern::lookup of csrc/scene_tables.hpp):
    rows sorted by length, longest first and stable; address = (slice_off[s] + 64 k) * 9 + lane for the k-th column of the row at position 64 s + lane"""
    rows = [{v} for v in range(NV)]
    for c in cliques:
        for a in c:
            rows[int(a)].update(int(x) for x in c)
    rows = [sorted(r) for r in rows]
    ln = np.array([len(r) for r in rows])
    perm = np.argsort(-ln, kind="stable")
    rowpos = np.empty(NV, np.int64); rowpos[perm] = np.arange(NV)
    n_slices = (NV + 63) // 64
    pad = np.zeros(64 * n_slices, np.int64); pad[:NV] = ln[perm]
    slice_off = np.concatenate([[0], np.cumsum(64 * pad.reshape(n_slices, 64).max(1))])
    out = {}
    for v, r in enumerate(rows):
        p = int(rowpos[v]); s, lane = p >> 6, p & 63
        for kk, c in enumerate(r):
            out[(v, c)] = int((slice_off[s] + 64 * kk) * 9 + lane)
    return out


def corner_lists(cv, address):
    """the lists of handle_lists (csrc/handle_host.hpp) for the corners cv (n x nc) as a dict of int arrays: the touched vertices ascending with their
    entries nc i + a ascending; the touched blocks ascending by (row vertex, column vertex) with their address and their entries nc nc i + nc a + b
    ascending"""
    cv = np.asarray(cv)
    n, nc = cv.shape
    by_v, by_b = {}, {}
    for i in range(n):
        for a in range(nc):
            by_v.setdefault(int(cv[i, a]), []).append(nc * i + a)
            for c in range(nc):
                by_b.setdefault((int(cv[i, a]), int(cv[i, c])), []).append(nc * nc * i + nc * a + c)
    vl_v, vl_ptr, vl_ent = [], [0], []
    for v in sorted(by_v):
        vl_v.append(v); vl_ent += sorted(by_v[v]); vl_ptr.append(len(vl_ent))
    bl_addr, bl_ptr, bl_ent = [], [0], []
    for pr in sorted(by_b):
        bl_addr.append(address[pr]); bl_ent += sorted(by_b[pr]); bl_ptr.append(len(bl_ent))
    return dict(vl_v=vl_v, vl_ptr=vl_ptr, vl_ent=vl_ent, bl_addr=bl_addr, bl_ptr=bl_ptr, bl_ent=bl_ent)


def gather_lists(NV, faces_tab, faces, address):
    """the corners fv (n x 3 flat) of a face list and its lists: corner_lists with nc = 3 -- entries 3 i + a and 9 i + 3 a + b"""
    fv = np.asarray(faces_tab).reshape(-1, 3)[np.asarray(faces)]
    return dict(fv=fv.ravel(), **corner_lists(fv, address))
