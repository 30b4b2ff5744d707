"""NumPy restatement of the StVK membrane of a cloth face ("cloth<i>.membrane" = 1, csrc/k_cloth.hpp): energy, gradient and the exact 9 x 9
Hessian per face, the rest shape Dm rebuilt from the three rest lengths, and assembly into dense arrays for small cloths.

Per face with vertices x0, x1, x2 (the edge order of k_cloth_grad_face: l0 = |x0 - x1|, l1 = |x1 - x2|, l2 = |x2 - x0|):
    Dm = [[l0, a], [0, b]], a = (l0^2 + l2^2 - l1^2) / (2 l0), b = sqrt(l2^2 - a^2)
    F = [x1 - x0, x2 - x0] Dm^-1,  E = (F^T F - I) / 2,  Psi = mu |E|_F^2 + lam/2 tr(E)^2,  energy A0 Psi.
"""
import numpy as np


def dm_from_lengths(l0, l1, l2):
    """Dm (2 x 2) of the rest triangle X0 = (0, 0), X1 = (l0, 0), X2 = (a, b)"""
    a = (l0 * l0 + l2 * l2 - l1 * l1) / (2.0 * l0)
    b = np.sqrt(l2 * l2 - a * a)
    return np.array([[l0, a], [0.0, b]])


def dminv_from_lengths(l0, l1, l2):
    return np.linalg.inv(dm_from_lengths(l0, l1, l2))


def _F(X, Di):
    Ds = np.stack([X[1] - X[0], X[2] - X[0]], 1)   # 3 x 2
    return Ds @ Di


def _B(Di):
    """b[v, j]: column j of F is sum_v b[v, j] x_v"""
    return np.array([-(Di[0] + Di[1]), Di[0], Di[1]])


def psi(F, mu, lam):
    E = 0.5 * (F.T @ F - np.eye(2))
    return mu * np.sum(E * E) + 0.5 * lam * np.trace(E) ** 2


def face_energy(X, Di, A0, mu, lam):
    return A0 * psi(_F(X, Di), mu, lam)


def face_grad(X, Di, A0, mu, lam):
    """3 x 3: the gradient at vertex v in row v"""
    F = _F(X, Di)
    E = 0.5 * (F.T @ F - np.eye(2))
    S = 2.0 * mu * E + lam * np.trace(E) * np.eye(2)
    P = F @ S                                      # 3 x 2
    return A0 * _B(Di) @ P.T


def dpsi2(F, mu, lam):
    """6 x 6 d2Psi / dF2, rows (column i of F, component a), columns (k, b)"""
    E = 0.5 * (F.T @ F - np.eye(2))
    S = 2.0 * mu * E + lam * np.trace(E) * np.eye(2)
    FFt = F @ F.T
    M = np.zeros((6, 6))
    for i in range(2):
        for k in range(2):
            blk = S[k, i] * np.eye(3) + mu * np.outer(F[:, k], F[:, i]) + lam * np.outer(F[:, i], F[:, k])
            if i == k:
                blk = blk + mu * FFt
            M[3 * i:3 * i + 3, 3 * k:3 * k + 3] = blk
    return M


def face_hess(X, Di, A0, mu, lam, clamp=False):
    """9 x 9 A0 B^T (d2Psi/dF2) B (rows 3 v + a); clamp: the 6 x 6 d2Psi/dF2 eigen-clamped first (spd 1)"""
    M = dpsi2(_F(X, Di), mu, lam)
    if clamp:
        w, V = np.linalg.eigh(0.5 * (M + M.T))
        M = (V * np.maximum(w, 0.0)) @ V.T
    b = _B(Di)
    Bm = np.zeros((6, 9))
    for j in range(2):
        for v in range(3):
            Bm[3 * j:3 * j + 3, 3 * v:3 * v + 3] = b[v, j] * np.eye(3)
    return A0 * Bm.T @ M @ Bm


# ------------------------------------------------------------------------------------------------ whole cloths
def grid_cloth(N, dx):
    """faces (init_mesh of the engine: f2v per cell (i, j), even cells (c, b, a), (a, d, c), odd (b, a, d), (d, c, b)), rest positions of an
    N x N grid in the xy plane, rest lengths (dx, dx, sqrt(2) dx) and rest areas dx^2 / 2"""
    f2v = []
    for i in range(N):
        for j in range(N):
            a = i * (N + 1) + j
            b, c, d = a + 1, a + N + 2, a + N + 1
            if (i + j) % 2 == 0:
                f2v += [(c, b, a), (a, d, c)]
            else:
                f2v += [(b, a, d), (d, c, b)]
    f2v = np.array(f2v, np.int64)
    ii, jj = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    X = np.stack([ii * dx, jj * dx, np.zeros(ii.shape)], -1).reshape(-1, 3).astype(np.float64)
    li = np.tile([dx, dx, dx * np.sqrt(2.0)], (len(f2v), 1))
    V = np.full(len(f2v), dx * dx * 0.5)
    return f2v, X, li, V


def dminv_all(li):
    return np.array([dminv_from_lengths(*l) for l in li])


def energy(x, f2v, Dis, V, mu, lam):
    return sum(face_energy(x[f], Di, A0, mu, lam) for f, Di, A0 in zip(f2v, Dis, V))


def gradient(x, f2v, Dis, V, mu, lam):
    g = np.zeros_like(x)
    for f, Di, A0 in zip(f2v, Dis, V):
        np.add.at(g, f, face_grad(x[f], Di, A0, mu, lam))
    return g


def hessian(x, f2v, Dis, V, mu, lam, clamp=False):
    n = 3 * len(x)
    H = np.zeros((n, n))
    for f, Di, A0 in zip(f2v, Dis, V):
        h = face_hess(x[f], Di, A0, mu, lam, clamp)
        idx = np.concatenate([np.arange(3 * v, 3 * v + 3) for v in f])
        H[np.ix_(idx, idx)] += h
    return H
