"""Dense NumPy restatement of the capsule colliders (csrc/k_capsule.hpp, csrc/capsule_host.hpp) for tests/test_capsule_numpy.py and
tests/test_gpu_capsules.py.

Capsule j: endpoints a_j, b_j, previous endpoints ap_j, bp_j (where the rod was at the start of the step), radius R_j, friction mu_j; shared
stiffness k, shell eps, friction regularisation eh = eps_v dt.  For vertex v with position x and start-of-step position x_prev:
  e  = b - a,    s  = (x - a) . e / (e . e),           t  = clamp(s, 0, 1),   in  = [0 < s < 1],   u  = e / |e|
  c  = a + t e,  q  = x - c,  rho = |q|,  n = q / rho,  d = rho - R
  e0 = bp - ap,  s0 = (x_prev - ap) . e0 / (e0 . e0),  t0 = clamp(s0, 0, 1),  in0 = [0 < s0 < 1],  u0 = e0 / |e0|
  c0 = ap + t0 e0,  q0 = x_prev - c0,  rho0, n0, d0 = rho0 - R
  lam = mu k max(0, eps - d0),  D = (x - x_prev) - ((1 - t0)(a - ap) + t0 (b - bp)),  P0 = I - n0 n0^T,  w = P0 D,  r = |w|,  a1 = f1(r)
  E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r),  g = [d < eps] k (d - eps) n + lam a1 w
  H = H_n + lam M,  H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T - in u u^T)),  M = a1 P0 + [r > 1e-9] (f2 / r) w w^T
The projected operator drops the second part of H_n.  A pair with rho < 1e-12 contributes nothing; one with rho0 < 1e-12 has no friction.
Everything here is written from these formulas with dense matrices and loops, not from the kernels; the gap is formed in extended precision.
The keyword `drop` takes one term out of the derivatives, for the sensitivity figures: "uu" (in u u^T in H_n), "tau_n" (phi' tau n^T in dg/da,
dg/db), "delta_dt0" (Delta dt0^T in the lagged columns), "tau0_n0" (the tau0 n0^T part of dn0/dap, dn0/dbp)."""
import numpy as np

from collider_numpy import f0, f1, f2   # the friction regularisation of k_contact.hpp, restated there

I3 = np.eye(3)
TINY = 1e-12
LD = np.longdouble


def full_mask(NV, n_cap):
    return np.full(NV, (1 << n_cap) - 1, np.uint8)


def mask_from_ids(NV, ids_per_capsule):
    m = np.zeros(NV, np.uint8)
    for j, ids in enumerate(ids_per_capsule):
        m[np.asarray(ids, np.int64)] |= np.uint8(1 << j)
    return m


def _closest(xv, aj, bj, Rj):
    """(e, e . e, s, t, in, x - c, |x - c|, |x - c| - R) in extended precision, rounded once at the end"""
    x, a, b = np.asarray(xv, LD), np.asarray(aj, LD), np.asarray(bj, LD)
    e = b - a
    ee = (e * e).sum()
    s = ((x - a) * e).sum() / ee
    t = min(max(s, LD(0)), LD(1))
    q = x - (a + t * e)
    rho = np.sqrt((q * q).sum())
    return e.astype(np.float64), float(ee), float(s), float(t), bool(0 < s < 1), q.astype(np.float64), float(rho), float(rho - LD(Rj))


class Pair:
    """the quantities of one (vertex, capsule) pair; ok False: rho < 1e-12, the pair contributes nothing"""

    def __init__(self, xv, xpv, a, b, ap, bp, Rj, muj, k, eps, eh, drop=None):
        self.drop = drop
        self.e, self.ee, self.s, self.t, self.inn, q, self.rho, self.d = _closest(xv, a, b, Rj)
        self.ok = self.rho >= TINY
        if not self.ok:
            return
        self.n = q / self.rho
        self.u = self.e / np.sqrt(self.ee)
        self.e0, self.ee0, self.s0, self.t0, self.in0, self.q0, self.rho0, self.d0 = _closest(xpv, ap, bp, Rj)
        self.u0 = self.e0 / np.sqrt(self.ee0)
        self.fric = self.rho0 >= TINY
        self.n0 = self.q0 / self.rho0 if self.fric else np.zeros(3)
        self.pen = max(0.0, eps - self.d0) if self.fric else 0.0
        self.lam = muj * k * self.pen
        self.P0 = I3 - np.outer(self.n0, self.n0)
        self.Delta = (b - bp) - (a - ap)
        self.D = (xv - xpv) - ((1.0 - self.t0) * (a - ap) + self.t0 * (b - bp))
        self.w = self.P0 @ self.D
        self.r = float(np.sqrt(self.w @ self.w))
        self.a1 = f1(self.r, eh)
        self.f2r = f2(self.r, eh) / self.r if self.r > 1e-9 else 0.0
        self.k, self.eps, self.eh, self.mu = k, eps, eh, muj
        self.act = self.d < eps
        self.act0 = self.fric and self.d0 < eps
        self.phi1 = k * (self.d - eps) if self.act else 0.0
        self.tau = self.e / self.ee if self.inn else np.zeros(3)
        self.tau0 = self.e0 / self.ee0 if self.in0 else np.zeros(3)

    def region(self):
        """(region of t, region of t0): -1 clamped low, 0 inside, 1 clamped high"""
        return (0 if self.inn else (-1 if self.s <= 0 else 1)), (0 if self.in0 else (-1 if self.s0 <= 0 else 1))

    def E(self):
        return (0.5 * self.k * (self.d - self.eps) ** 2 if self.act else 0.0) + self.lam * f0(self.r, self.eh)

    def g(self):
        return (self.k * (self.d - self.eps) * self.n if self.act else np.zeros(3)) + self.lam * self.a1 * self.w

    def curvature(self):
        """the part of H_n that the projected modes leave out"""
        if not self.act:
            return np.zeros((3, 3))
        G = I3 - np.outer(self.n, self.n)
        if self.inn and self.drop != "uu":
            G = G - np.outer(self.u, self.u)
        return self.k * (self.d - self.eps) / self.rho * G

    def Hn(self, exact=True):
        if not self.act:
            return np.zeros((3, 3))
        H = self.k * np.outer(self.n, self.n)
        return H + self.curvature() if exact else H

    def M(self):
        return self.a1 * self.P0 + self.f2r * np.outer(self.w, self.w)

    def B(self):
        return self.a1 * I3 + self.f2r * np.outer(self.w, self.w)

    # ---- derivatives of g
    def dg_da(self):
        tn = np.zeros((3, 3)) if self.drop == "tau_n" else self.phi1 * np.outer(self.tau, self.n)
        return -(1.0 - self.t) * self.Hn() + tn - (1.0 - self.t0) * self.lam * self.M()

    def dg_db(self):
        tn = np.zeros((3, 3)) if self.drop == "tau_n" else self.phi1 * np.outer(self.tau, self.n)
        return -self.t * self.Hn() - tn - self.t0 * self.lam * self.M()

    def lagged(self, dd0, dn0, dt0, dD):
        """dd0 (3): d(d0)/d(parameter); dn0 (3 x 3): d(n0)/d(parameter); dt0 (3): d(t0)/d(parameter); dD (3 x 3): d(D)/d(parameter) at fixed t0"""
        if not self.fric:
            return np.zeros((3, 3))
        out = np.zeros((3, 3))
        if self.act0:
            out -= self.mu * self.k * np.outer(self.a1 * self.w, dd0)
        Jn = -self.B() @ (float(self.n0 @ self.D) * I3 + np.outer(self.n0, self.D))
        dDt = dD if self.drop == "delta_dt0" else dD - np.outer(self.Delta, dt0)
        return out + self.lam * (self.M() @ dDt + Jn @ dn0)

    def G0(self):
        G = self.P0.copy()
        if self.in0:
            G -= np.outer(self.u0, self.u0)
        return G

    def dg_dxp(self):
        if not self.fric:
            return np.zeros((3, 3))
        return self.lagged(self.n0, self.G0() / self.rho0, self.tau0, -I3)

    def dg_dap(self):
        if not self.fric:
            return np.zeros((3, 3))
        tn = np.zeros((3, 3)) if self.drop == "tau0_n0" else np.outer(self.tau0, self.n0)
        dt0 = (-self.q0 - (1.0 - self.s0) * self.e0) / self.ee0 if self.in0 else np.zeros(3)
        return self.lagged(-(1.0 - self.t0) * self.n0, -(1.0 - self.t0) * self.G0() / self.rho0 + tn, dt0, (1.0 - self.t0) * I3)

    def dg_dbp(self):
        if not self.fric:
            return np.zeros((3, 3))
        tn = np.zeros((3, 3)) if self.drop == "tau0_n0" else np.outer(self.tau0, self.n0)
        dt0 = (self.q0 - self.s0 * self.e0) / self.ee0 if self.in0 else np.zeros(3)
        return self.lagged(-self.t0 * self.n0, -self.t0 * self.G0() / self.rho0 - tn, dt0, self.t0 * I3)

    def dR(self):
        return (-self.k * self.n if self.act else np.zeros(3)) + (self.mu * self.k * self.a1 * self.w if self.act0 else np.zeros(3))

    def dmu(self):
        return self.k * self.pen * self.a1 * self.w


def pairs(x, xp, a, b, ap, bp, R, mu, mask, k, eps, eh, drop=None):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    xp = np.asarray(xp, np.float64).reshape(-1, 3)
    for v in range(len(x)):
        for j in range(len(R)):
            if (int(mask[v]) >> j) & 1:
                P = Pair(x[v], xp[v], a[j], b[j], ap[j], bp[j], R[j], mu[j], k, eps, eh, drop)
                if P.ok:
                    yield v, j, P


def _nv(x):
    return len(np.asarray(x).reshape(-1, 3))


def energy(x, xp, *A, **kw):
    return sum(P.E() for v, j, P in pairs(x, xp, *A, **kw))


def gradient(x, xp, *A, **kw):
    """(NV, 3) dE/dx"""
    g = np.zeros((_nv(x), 3))
    for v, j, P in pairs(x, xp, *A, **kw):
        g[v] += P.g()
    return g


def blocks(x, xp, *A, exact=True, **kw):
    """(NV, 3, 3): the diagonal blocks; exact: the reverse step's operator (spd = 0), else the projected one of every other mode"""
    H = np.zeros((_nv(x), 3, 3))
    for v, j, P in pairs(x, xp, *A, **kw):
        H[v] += P.Hn(exact) + P.lam * P.M()
    return H


def curvature_blocks(x, xp, *A):
    """(NV, 3, 3): exact minus projected"""
    H = np.zeros((_nv(x), 3, 3))
    for v, j, P in pairs(x, xp, *A):
        H[v] += P.curvature()
    return H


def hessian(x, xp, *A, exact=True, **kw):
    """dense (3 NV, 3 NV)"""
    B = blocks(x, xp, *A, exact=exact, **kw)
    H = np.zeros((3 * len(B), 3 * len(B)))
    for v in range(len(B)):
        H[3 * v:3 * v + 3, 3 * v:3 * v + 3] = B[v]
    return H


def force(x, xp, a, b, *rest):
    """(n_cap, 6): -sum_v g_v of every capsule and -sum_v (x_v - m) x g_v about its midpoint m = (a + b) / 2 (frozen dofs not masked)"""
    xs = np.asarray(x, np.float64).reshape(-1, 3)
    F = np.zeros((len(a), 6))
    for v, j, P in pairs(x, xp, a, b, *rest):
        g = P.g()
        F[j, 0:3] -= g
        F[j, 3:6] -= np.cross(xs[v] - 0.5 * (a[j] + b[j]), g)
    return F


def _free(frozen, p):
    free = (np.asarray(frozen).reshape(-1, 3) == 0).astype(np.float64)
    return free, np.asarray(p, np.float64).reshape(-1, 3) * free


def backprop_prev(x, xp, p, frozen, *A, **kw):
    """(NV, 3): what a reverse step adds to pos_grad[s-1]: -(dg/dx_prev)^T p_v on the free dofs, p's frozen dofs not counting"""
    free, p = _free(frozen, p)
    out = np.zeros_like(p)
    for v, j, P in pairs(x, xp, *A, **kw):
        out[v] -= P.dg_dxp().T @ p[v]
    return out * free


def capsule_grad(x, xp, p, frozen, *A, **kw):
    """(n_cap, 14): the shares of one reverse step in d(loss)/d(a_j, b_j, ap_j, bp_j, mu_j, R_j)"""
    free, p = _free(frozen, p)
    G = np.zeros((len(A[0]), 14))
    for v, j, P in pairs(x, xp, *A, **kw):
        G[j, 0:3] -= P.dg_da().T @ p[v]
        G[j, 3:6] -= P.dg_db().T @ p[v]
        G[j, 6:9] -= P.dg_dap().T @ p[v]
        G[j, 9:12] -= P.dg_dbp().T @ p[v]
        G[j, 12] -= float(p[v] @ P.dmu())
        G[j, 13] -= float(p[v] @ P.dR())
    return G


def active_sets(x, xp, *A):
    """(NV, n_cap) arrays over the masked pairs: d < eps, d0 < eps, the region of t and of t0 (-1, 0, 1; 9 where the pair is masked out)"""
    NV, n = _nv(x), len(A[4])
    act, act0 = np.zeros((NV, n), bool), np.zeros((NV, n), bool)
    reg, reg0 = np.full((NV, n), 9), np.full((NV, n), 9)
    for v, j, P in pairs(x, xp, *A):
        act[v, j], act0[v, j] = P.act, P.act0
        reg[v, j], reg0[v, j] = P.region()
    return act, act0, reg, reg0
