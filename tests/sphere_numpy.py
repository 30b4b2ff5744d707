"""Dense NumPy restatement of the sphere colliders (csrc/k_sphere.hpp, csrc/sphere_host.hpp) for tests/test_sphere_numpy.py and
tests/test_gpu_spheres.py.

Sphere j: centre c_j, previous centre cp_j (where the ball was at the start of the step), radius R_j, friction mu_j; shared stiffness k, shell
eps, friction regularisation eh = eps_v dt.  For vertex v with position x and start-of-step position x_prev:
  q  = x - c,       rho  = |q|,  n  = q / rho,   d  = rho - R
  q0 = x_prev - cp, rho0 = |q0|, n0 = q0 / rho0, d0 = rho0 - R
  lam = mu k max(0, eps - d0),  P0 = I - n0 n0^T,  D = (x - x_prev) - (c - cp),  w = P0 D,  r = |w|,  a = f1(r)
  E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r),  g = [d < eps] k (d - eps) n + lam a w
  H = H_n + lam M,  H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T)),  M = a P0 + [r > 1e-9] (f2 / r) w w^T
The projected operator drops the second part of H_n.  A pair with rho < 1e-12 contributes nothing; one with rho0 < 1e-12 has no friction.
Everything here is written from these formulas with dense arrays and loops, not from the kernels."""
import numpy as np

from collider_numpy import f0, f1, f2   # the friction regularisation of k_contact.hpp, restated there

I3 = np.eye(3)
TINY = 1e-12


def full_mask(NV, n_sph):
    return np.full(NV, (1 << n_sph) - 1, np.uint8)


def mask_from_ids(NV, ids_per_sphere):
    m = np.zeros(NV, np.uint8)
    for j, ids in enumerate(ids_per_sphere):
        m[np.asarray(ids, np.int64)] |= np.uint8(1 << j)
    return m


def _pairs(x, xp, c, mask):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    xp = np.asarray(xp, np.float64).reshape(-1, 3)
    for v in range(len(x)):
        for j in range(len(c)):
            if (int(mask[v]) >> j) & 1:
                yield v, j, x[v], xp[v]


def _gap(xv, cj, Rj):
    """(x - c, |x - c|, |x - c| - R); the gap in extended precision, rounded once: the kernels form it without its cancellations (sph_gap)"""
    q = np.asarray(xv, np.longdouble) - np.asarray(cj, np.longdouble)
    rho = np.sqrt((q * q).sum())
    return q.astype(np.float64), float(rho), float(rho - np.longdouble(Rj))


class Pair:
    """the quantities of one (vertex, sphere) pair; ok False: rho < 1e-12, the pair contributes nothing"""

    def __init__(self, xv, xpv, cj, cpj, Rj, muj, k, eps, eh, drop_centre_motion=False):
        q, self.rho, self.d = _gap(xv, cj, Rj)
        self.ok = self.rho >= TINY
        if not self.ok:
            return
        self.n = q / self.rho
        q0, self.rho0, self.d0 = _gap(xpv, cpj, Rj)
        self.fric = self.rho0 >= TINY
        self.n0 = q0 / self.rho0 if self.fric else np.zeros(3)
        self.pen = max(0.0, eps - self.d0) if self.fric else 0.0
        self.lam = muj * k * self.pen
        self.P0 = I3 - np.outer(self.n0, self.n0)
        self.D = (xv - xpv) - (0.0 if drop_centre_motion else (cj - cpj))
        self.w = self.P0 @ self.D
        self.r = float(np.sqrt(self.w @ self.w))
        self.a = f1(self.r, eh)
        self.f2r = f2(self.r, eh) / self.r if self.r > 1e-9 else 0.0
        self.k, self.eps, self.eh, self.mu = k, eps, eh, muj
        self.act = self.d < eps
        self.act0 = self.fric and self.d0 < eps

    def E(self):
        return (0.5 * self.k * (self.d - self.eps) ** 2 if self.act else 0.0) + self.lam * f0(self.r, self.eh)

    def g(self):
        return (self.k * (self.d - self.eps) * self.n if self.act else np.zeros(3)) + self.lam * self.a * self.w

    def Hn(self, exact=True, curvature=True):
        if not self.act:
            return np.zeros((3, 3))
        nn = np.outer(self.n, self.n)
        H = self.k * nn
        if exact and curvature:
            H = H + self.k * (self.d - self.eps) / self.rho * (I3 - nn)
        return H

    def M(self):
        return self.a * self.P0 + self.f2r * np.outer(self.w, self.w)

    def B(self):
        return self.a * I3 + self.f2r * np.outer(self.w, self.w)

    def L(self, with_Jn=True):
        """dg / d(q0) at fixed D"""
        if not self.fric:
            return np.zeros((3, 3))
        out = np.zeros((3, 3))
        if self.act0:
            out -= self.mu * self.k * np.outer(self.a * self.w, self.n0)
        if with_Jn:
            Jn = -self.B() @ (float(self.n0 @ self.D) * I3 + np.outer(self.n0, self.D))
            out += self.lam * (Jn @ self.P0) / self.rho0
        return out

    def dR(self):
        return (-self.k * self.n if self.act else np.zeros(3)) + (self.mu * self.k * self.a * self.w if self.act0 else np.zeros(3))

    def dmu(self):
        return self.k * self.pen * self.a * self.w


def pairs(x, xp, c, cp, R, mu, mask, k, eps, eh, **kw):
    for v, j, xv, xpv in _pairs(x, xp, c, mask):
        P = Pair(xv, xpv, c[j], cp[j], R[j], mu[j], k, eps, eh, **kw)
        if P.ok:
            yield v, j, P


def _nv(x):
    return len(np.asarray(x).reshape(-1, 3))


def energy(x, xp, c, cp, R, mu, mask, k, eps, eh, **kw):
    return sum(P.E() for v, j, P in pairs(x, xp, c, cp, R, mu, mask, k, eps, eh, **kw))


def gradient(x, xp, c, cp, R, mu, mask, k, eps, eh, **kw):
    """(NV, 3) dE/dx"""
    g = np.zeros((_nv(x), 3))
    for v, j, P in pairs(x, xp, c, cp, R, mu, mask, k, eps, eh, **kw):
        g[v] += P.g()
    return g


def blocks(x, xp, c, cp, R, mu, mask, k, eps, eh, exact=True, curvature=True):
    """(NV, 3, 3): the diagonal blocks; exact: the reverse step's operator (spd = 0), else the projected one of every other mode"""
    H = np.zeros((_nv(x), 3, 3))
    for v, j, P in pairs(x, xp, c, cp, R, mu, mask, k, eps, eh):
        H[v] += P.Hn(exact, curvature) + P.lam * P.M()
    return H


def hessian(x, xp, c, cp, R, mu, mask, k, eps, eh, exact=True, curvature=True):
    """dense (3 NV, 3 NV)"""
    B = blocks(x, xp, c, cp, R, mu, mask, k, eps, eh, exact, curvature)
    H = np.zeros((3 * len(B), 3 * len(B)))
    for v in range(len(B)):
        H[3 * v:3 * v + 3, 3 * v:3 * v + 3] = B[v]
    return H


def force(x, xp, c, cp, R, mu, mask, k, eps, eh):
    """(n_sph, 3): -sum_v g_v of every sphere (frozen dofs not masked)"""
    F = np.zeros((len(c), 3))
    for v, j, P in pairs(x, xp, c, cp, R, mu, mask, k, eps, eh):
        F[j] -= P.g()
    return F


def _free(frozen, p):
    free = (np.asarray(frozen).reshape(-1, 3) == 0).astype(np.float64)
    return free, np.asarray(p, np.float64).reshape(-1, 3) * free


def backprop_prev(x, xp, p, frozen, c, cp, R, mu, mask, k, eps, eh, with_Jn=True, **kw):
    """(NV, 3): what a reverse step adds to pos_grad[s-1]: -(dg/dx_prev)^T p_v = lam M p_v - L^T p_v on the free dofs, p's frozen dofs not counting"""
    free, p = _free(frozen, p)
    out = np.zeros_like(p)
    for v, j, P in pairs(x, xp, c, cp, R, mu, mask, k, eps, eh, **kw):
        out[v] += P.lam * (P.M() @ p[v]) - P.L(with_Jn).T @ p[v]
    return out * free


def sphere_grad(x, xp, p, frozen, c, cp, R, mu, mask, k, eps, eh):
    """(n_sph, 8): the shares of one reverse step in d(loss)/d(c_j), d(loss)/d(cp_j), d(loss)/d(mu_j), d(loss)/d(R_j)"""
    free, p = _free(frozen, p)
    G = np.zeros((len(c), 8))
    for v, j, P in pairs(x, xp, c, cp, R, mu, mask, k, eps, eh):
        dg_dc = -(P.Hn(True) + P.lam * P.M())
        dg_dcp = P.lam * P.M() - P.L()
        G[j, 0:3] -= dg_dc.T @ p[v]
        G[j, 3:6] -= dg_dcp.T @ p[v]
        G[j, 6] -= float(p[v] @ P.dmu())
        G[j, 7] -= float(p[v] @ P.dR())
    return G


def active_sets(x, xp, c, cp, R, mask, eps):
    """two boolean (NV, n_sph) arrays: d < eps and d0 < eps on the masked pairs"""
    x = np.asarray(x, np.float64).reshape(-1, 3); xp = np.asarray(xp, np.float64).reshape(-1, 3)
    on = ((np.asarray(mask)[:, None].astype(np.int64) >> np.arange(len(c))[None, :]) & 1).astype(bool)
    d = np.linalg.norm(x[:, None, :] - c[None, :, :], axis=2) - R[None, :]
    d0 = np.linalg.norm(xp[:, None, :] - cp[None, :, :], axis=2) - R[None, :]
    return (d < eps) & on, (d0 < eps) & on
