"""NumPy restatement of the soft-handle term (csrc/k_handle.hpp): handle i ties vertex v_i to a world-space target t_i,

    E_h = 1/2 k sum_i w_i |x_{v_i} - t_i|^2.

Frozen rule (the engine's mask rule, BaseScene.py:399-405 of the reference): a frozen dof has no gradient entry, no matrix row or column of the
term, and contributes to no gradient with respect to a target or to k.  The energy and the force read-out are not masked."""
import numpy as np


def _free(frozen, NV):
    return np.ones((NV, 3), bool) if frozen is None else ~np.asarray(frozen).reshape(NV, 3).astype(bool)


def energy(x, v, w, t, k):
    d = x[v] - t
    return 0.5 * k * float((w * (d * d).sum(1)).sum())


def gradient(x, v, w, t, k, frozen=None):
    """(NV, 3): row v_i = k w_i (x - t_i), zero on frozen dofs"""
    g = np.zeros_like(x)
    g[v] = k * w[:, None] * (x[v] - t)
    return g * _free(frozen, len(x))


def diagonal(NV, v, w, k, frozen=None):
    """(NV, 3): the term's entries on the matrix diagonal, k w_i on the three dofs of v_i (nothing else of the matrix is touched), zero on frozen dofs"""
    d = np.zeros((NV, 3))
    d[v] = (k * w)[:, None]
    return d * _free(frozen, NV)


def force(x, v, w, t, k):
    """(n, 3): k w_i (t_i - x_{v_i}), the force the handle applies to the cloth; not masked"""
    return k * w[:, None] * (t - x[v])


def target_grad(p, v, w, k, frozen=None):
    """(n, 3): -p . dF/dt_i = k w_i p_{v_i} on free dofs, 0 on frozen ones (F the masked gradient)"""
    p = p.reshape(-1, 3)
    return k * w[:, None] * p[v] * _free(frozen, len(p))[v]


def k_deriv(x, p, v, w, t, frozen=None):
    """-p . dF/dk over the free dofs = -sum_i w_i p_{v_i} . (x_{v_i} - t_i)"""
    p = p.reshape(-1, 3)
    return -float((w[:, None] * p[v] * (x[v] - t) * _free(frozen, len(x))[v]).sum())
