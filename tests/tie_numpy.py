"""Dense NumPy restatement of the ties (csrc/k_tie.hpp, csrc/tie_host.hpp) for tests/test_tie_numpy.py and tests/test_gpu_ties.py.

Tie i binds vertex v_i to the point with barycentric coordinates b_i on face (t0, t1, t2): r_i = x_v - sum_a b_a x_{t_a},
E = 1/2 k sum_i w_i |r_i|^2.  In the slot order (t0, t1, t2, v) with c = (-b0, -b1, -b2, 1) the gradient on corner a is k w_i c_a r_i and the
12 x 12 block k w_i (c c^T) (x) I_3.  Everything here is written from these formulas with dense arrays, not from the kernels."""
import numpy as np


def records(faces_tab, verts, faces, bary, weights=None):
    """(idx (n, 4) = (t0, t1, t2, v), b (n, 3), w (n)): the slot records of a list"""
    faces_tab = np.asarray(faces_tab).reshape(-1, 3)
    verts = np.asarray(verts, np.int64).reshape(-1)
    faces = np.asarray(faces, np.int64).reshape(-1)
    idx = np.concatenate([faces_tab[faces], verts[:, None]], axis=1).astype(np.int64).reshape(-1, 4)
    b = np.asarray(bary, np.float64).reshape(-1, 3)
    w = np.ones(len(verts)) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    return idx, b, w


def coeffs(b):
    """(n, 4): c = (-b0, -b1, -b2, 1)"""
    return np.concatenate([-b, np.ones((len(b), 1))], axis=1)


def residuals(x, idx, b):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    return np.einsum("ia,iad->id", coeffs(b), x[idx])


def energy(x, idx, b, w, k):
    r = residuals(x, idx, b)
    return 0.5 * k * float(np.sum(w * np.sum(r * r, axis=1)))


def gradient(x, idx, b, w, k):
    """(NV, 3) dE/dx"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    r = residuals(x, idx, b)
    g = np.zeros_like(x)
    c = coeffs(b)
    for i in range(len(idx)):
        for a in range(4):
            g[idx[i, a]] += k * w[i] * c[i, a] * r[i]
    return g


def blocks(b, w, k):
    """(n, 12, 12): k w_i (c c^T) (x) I_3"""
    c = coeffs(b)
    return np.stack([k * w[i] * np.kron(np.outer(c[i], c[i]), np.eye(3)) for i in range(len(b))]) if len(b) else np.zeros((0, 12, 12))


def hessian(NV, idx, b, w, k):
    """dense (3 NV, 3 NV)"""
    H = np.zeros((3 * NV, 3 * NV))
    B = blocks(b, w, k)
    for i in range(len(idx)):
        d = np.concatenate([3 * v + np.arange(3) for v in idx[i]])
        H[np.ix_(d, d)] += B[i]
    return H


def force(x, idx, b, w, k):
    """(n, 3) -k w_i r_i: the force on the vertex of every tie"""
    return -k * w[:, None] * residuals(x, idx, b)


def pg_rows(x, p, frozen, idx, b):
    """(n,) g_i = -sum_a sum_{c free} p_{a, c} c_a r_{i, c}: tie_grad is k g_i, the k_tie key sum_i w_i g_i"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    free = (np.asarray(frozen).reshape(-1, 3) == 0).astype(np.float64)
    r = residuals(x, idx, b)
    c = coeffs(b)
    return -np.einsum("ia,iad,iad,id->i", c, p[idx], free[idx], r)
