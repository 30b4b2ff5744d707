"""Dense NumPy restatement of the half-space colliders (csrc/k_collider.hpp, csrc/collider_host.hpp) for tests/test_collider_numpy.py
and tests/test_gpu_colliders.py.

Collider j: unit normal n_j, offset o_j (solid side n . x < o), friction mu_j; shared stiffness k, shell eps, friction regularisation eh = eps_v dt.
For vertex v with position x and start-of-step position x_prev:
  d = n . x - o, d0 = n . x_prev - o, lam = mu k max(0, eps - d0), u = T^T (x - x_prev), r = |u|,
  E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r),  g = [d < eps] k (d - eps) n + lam f1(r) T u,
  H = [d < eps] k n n^T + lam T (f1 I + [r > 1e-9] (f2 / r) u u^T) T^T.
Everything here is written from these formulas with dense arrays and loops, not from the kernels."""
import numpy as np


def f0(x, eh):
    return x if x > eh else -x ** 3 / (3.0 * eh * eh) + x * x / eh + eh / 3.0


def f1(x, eh):
    return 1.0 / x if x > eh else -x / (eh * eh) + 2.0 / eh


def f2(x, eh):
    return -1.0 / (x * x) if x > eh else -1.0 / (eh * eh)


def unit(normals):
    n = np.asarray(normals, np.float64).reshape(-1, 3)
    return n / np.linalg.norm(n, axis=1)[:, None]


def tangents(n):
    """(t1, t2) of a unit normal, as the contact pairs build theirs: t1 = |n.x| < 0.5 ? (n.x, n.z, -n.y) : (n.y, -n.x, n.z); t2 = n x t1; t1 = n x t2"""
    t1 = np.array([n[0], n[2], -n[1]]) if abs(n[0]) < 0.5 else np.array([n[1], -n[0], n[2]])
    t2 = np.cross(n, t1)
    t1 = np.cross(n, t2)
    return t1, t2


def full_mask(NV, n_col):
    return np.full(NV, (1 << n_col) - 1, np.uint8)


def mask_from_ids(NV, ids_per_collider):
    m = np.zeros(NV, np.uint8)
    for j, ids in enumerate(ids_per_collider):
        m[np.asarray(ids, np.int64)] |= np.uint8(1 << j)
    return m


def _pairs(x, xp, n, o, mu, mask):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    xp = np.asarray(xp, np.float64).reshape(-1, 3)
    for v in range(len(x)):
        for j in range(len(n)):
            if (int(mask[v]) >> j) & 1:
                yield v, j, x[v], xp[v]


def _terms(xv, xpv, nj, oj, muj, k, eps, eh):
    t1, t2 = tangents(nj)
    T = np.stack([t1, t2], axis=1)   # 3 x 2
    d = float(nj @ xv - oj); d0 = float(nj @ xpv - oj)
    pen = max(0.0, eps - d0)
    lam = muj * k * pen
    u = T.T @ (xv - xpv)
    r = float(np.sqrt(u @ u))
    return T, d, d0, pen, lam, u, r


def energy(x, xp, n, o, mu, mask, k, eps, eh):
    E = 0.0
    for v, j, xv, xpv in _pairs(x, xp, n, o, mu, mask):
        T, d, d0, pen, lam, u, r = _terms(xv, xpv, n[j], o[j], mu[j], k, eps, eh)
        if d < eps:
            E += 0.5 * k * (d - eps) ** 2
        E += lam * f0(r, eh)
    return E


def pair_gradient(xv, xpv, nj, oj, muj, k, eps, eh):
    T, d, d0, pen, lam, u, r = _terms(xv, xpv, nj, oj, muj, k, eps, eh)
    g = np.zeros(3)
    if d < eps:
        g += k * (d - eps) * nj
    g += lam * f1(r, eh) * (T @ u)
    return g


def gradient(x, xp, n, o, mu, mask, k, eps, eh):
    """(NV, 3) dE/dx"""
    g = np.zeros((len(np.asarray(x).reshape(-1, 3)), 3))
    for v, j, xv, xpv in _pairs(x, xp, n, o, mu, mask):
        g[v] += pair_gradient(xv, xpv, n[j], o[j], mu[j], k, eps, eh)
    return g


def friction_block(T, lam, u, r, eh):
    core = f1(r, eh) * np.eye(2)
    if r > 1e-9:
        core = core + (f2(r, eh) / r) * np.outer(u, u)
    return lam * (T @ core @ T.T)


def blocks(x, xp, n, o, mu, mask, k, eps, eh):
    """(NV, 3, 3): the diagonal blocks H_v"""
    H = np.zeros((len(np.asarray(x).reshape(-1, 3)), 3, 3))
    for v, j, xv, xpv in _pairs(x, xp, n, o, mu, mask):
        T, d, d0, pen, lam, u, r = _terms(xv, xpv, n[j], o[j], mu[j], k, eps, eh)
        if d < eps:
            H[v] += k * np.outer(n[j], n[j])
        H[v] += friction_block(T, lam, u, r, eh)
    return H


def hessian(x, xp, n, o, mu, mask, k, eps, eh):
    """dense (3 NV, 3 NV)"""
    B = blocks(x, xp, n, o, mu, mask, k, eps, eh)
    H = np.zeros((3 * len(B), 3 * len(B)))
    for v in range(len(B)):
        H[3 * v:3 * v + 3, 3 * v:3 * v + 3] = B[v]
    return H


def force(x, xp, n, o, mu, mask, k, eps, eh):
    """(n_col, 3): -sum_v g_v of every collider (frozen dofs not masked)"""
    F = np.zeros((len(n), 3))
    for v, j, xv, xpv in _pairs(x, xp, n, o, mu, mask):
        F[j] -= pair_gradient(xv, xpv, n[j], o[j], mu[j], k, eps, eh)
    return F


def backprop_prev(x, xp, p, frozen, n, o, mu, mask, k, eps, eh):
    """(NV, 3): what a reverse step adds to pos_grad[s-1]: H_f p_v + [d0 < eps] mu k (p_v . f1 T u) n on the free dofs, p's frozen dofs not counting"""
    free = (np.asarray(frozen).reshape(-1, 3) == 0).astype(np.float64)
    p = np.asarray(p, np.float64).reshape(-1, 3) * free
    out = np.zeros_like(p)
    for v, j, xv, xpv in _pairs(x, xp, n, o, mu, mask):
        T, d, d0, pen, lam, u, r = _terms(xv, xpv, n[j], o[j], mu[j], k, eps, eh)
        out[v] += friction_block(T, lam, u, r, eh) @ p[v]
        if d0 < eps:
            out[v] += mu[j] * k * float(p[v] @ (f1(r, eh) * (T @ u))) * n[j]
    return out * free


def collider_grad(x, xp, p, frozen, n, o, mu, mask, k, eps, eh):
    """(n_col, 2): the shares of one reverse step in d(loss)/d(o_j) and d(loss)/d(mu_j)"""
    free = (np.asarray(frozen).reshape(-1, 3) == 0).astype(np.float64)
    p = np.asarray(p, np.float64).reshape(-1, 3) * free
    G = np.zeros((len(n), 2))
    for v, j, xv, xpv in _pairs(x, xp, n, o, mu, mask):
        T, d, d0, pen, lam, u, r = _terms(xv, xpv, n[j], o[j], mu[j], k, eps, eh)
        w = f1(r, eh) * (T @ u)
        dg_do = np.zeros(3)
        if d < eps:
            dg_do -= k * n[j]
        if d0 < eps:
            dg_do += mu[j] * k * w
        G[j, 0] -= float(p[v] @ dg_do)
        G[j, 1] -= float(p[v] @ (k * pen * w))
    return G


def active_sets(x, xp, n, o, mask, eps):
    """two boolean (NV, n_col) arrays: d < eps and d0 < eps on the masked pairs"""
    x = np.asarray(x, np.float64).reshape(-1, 3); xp = np.asarray(xp, np.float64).reshape(-1, 3)
    on = ((np.asarray(mask)[:, None].astype(np.int64) >> np.arange(len(n))[None, :]) & 1).astype(bool)
    return ((x @ n.T - o[None, :]) < eps) & on, ((xp @ n.T - o[None, :]) < eps) & on
