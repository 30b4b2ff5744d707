"""Dense NumPy restatement of the sampled distance-field colliders (csrc/k_sdf.hpp, csrc/sdf_host.hpp) for tests/test_sdf_numpy.py
and tests/test_gpu_sdfs.py.

Field j: samples s (n0, n1, n2), spacing h, origin o (local position of sample (0, 0, 0)); offset r, friction mu; centre c, rotation matrix R, previous
pose cp, R0; shared stiffness k, shell eps, friction regularisation eh = eps_v dt.  phi is the tensor-product uniform cubic B-spline with the samples
as control values:
  t = (y - o) / h,  i = floor(t),  f = t - i,   valid  <=>  1 <= t_a < n_a - 2 for every axis
  phi(y) = sum_{abc} B_a(f_0) B_b(f_1) B_c(f_2) s[i_0-1+a, i_1-1+b, i_2-1+c]
For vertex v with position x and start-of-step position x_prev:
  y  = R^T (x - c),        d  = phi(y) - r,    m  = R grad phi(y)
  y0 = R0^T (x_prev - cp), d0 = phi(y0) - r,   s0 = |grad phi(y0)|,  n0 = R0 grad phi(y0) / s0
  lam = [y0 valid][s0 >= 1e-12] mu k max(0, eps - d0),  D = (x - c) - R y0,  P0 = I - n0 n0^T,  w = P0 D,  r_w = |w|,  a1 = f1(r_w)
  E = [y valid][d < eps] 1/2 k (d - eps)^2 + lam f0(r_w),  g = [y valid][d < eps] k (d - eps) m + lam a1 w
  H = H_n + lam M,  H_n = [y valid][d < eps] k (m m^T + (d - eps) R Hess phi(y) R^T),  M = a1 P0 + [r_w > 1e-9] (f2 / r_w) w w^T
The projected operator drops the second part of H_n.  Everything here is written from these formulas with dense tensors (einsum over the 4 x 4 x 4
neighbourhood) and loops, not from the kernels.  The derivatives are the dense Jacobians dg/d(parameter); a rotation parameter is a world-frame
rotation vector applied on the left, R <- exp([theta]x) R.  The keyword `drop` takes one term out of the derivatives, for the mutation checks:
"hess0" (the term through Hess phi(y0) in the lagged columns), "curv" (the curvature part of H_n)."""
import numpy as np

from box_numpy import I3, quat_to_R, rot, skew   # noqa: F401  (the pose conventions are the boxes')
from collider_numpy import f0, f1, f2            # the friction regularisation of k_contact.hpp, restated there

TINY = 1e-12


def bspline(f):
    """(3, 4): the four weights B_a(f) and their first and second derivatives in f"""
    g = 1.0 - f
    return np.array([[g ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6],
                     [-g ** 2 / 2, (9 * f ** 2 - 12 * f) / 6, (-9 * f ** 2 + 6 * f + 3) / 6, f ** 2 / 2],
                     [g, 3 * f - 2, -3 * f + 1, f]])


class Field:
    def __init__(self, grid, origin, h):
        self.s = np.ascontiguousarray(grid, np.float64)
        assert self.s.ndim == 3
        self.o = np.asarray(origin, np.float64).reshape(3)
        self.h = float(h)

    @property
    def dims(self):
        return self.s.shape

    def coords(self, y):
        return (np.asarray(y, np.float64) - self.o) / self.h

    def valid(self, y):
        t = self.coords(y)
        return bool(all(t[a] >= 1.0 and t[a] < self.s.shape[a] - 2 for a in range(3)))   # (NaN fails both comparisons)

    def sample(self, y):
        """(phi, grad phi (3), Hess phi (3, 3)) at the local point y, or None outside the valid region"""
        if not self.valid(y):
            return None
        t = self.coords(y)
        i = np.floor(t).astype(np.int64)
        W = [bspline(t[a] - i[a]) for a in range(3)]
        blk = self.s[i[0] - 1:i[0] + 3, i[1] - 1:i[1] + 3, i[2] - 1:i[2] + 3]
        ev = lambda p, q, r: float(np.einsum("a,b,c,abc->", W[0][p], W[1][q], W[2][r], blk))
        phi = ev(0, 0, 0)
        g = np.array([ev(1, 0, 0), ev(0, 1, 0), ev(0, 0, 1)]) / self.h
        H = np.array([[ev(2, 0, 0), ev(1, 1, 0), ev(1, 0, 1)], [ev(1, 1, 0), ev(0, 2, 0), ev(0, 1, 1)], [ev(1, 0, 1), ev(0, 1, 1), ev(0, 0, 2)]]) / self.h ** 2
        return phi, g, H


def full_mask(NV, n):
    return np.full(NV, (1 << n) - 1, np.uint8)


class Pair:
    """the quantities of one (vertex, field) pair"""

    def __init__(self, xv, xpv, F, c, R, cp, R0, r, muj, k, eps, eh, drop=None):
        self.drop = drop
        self.x, self.xp, self.c, self.R, self.cp, self.R0 = (np.asarray(a, np.float64) for a in (xv, xpv, c, R, cp, R0))
        self.k, self.eps, self.eh, self.mu = k, eps, eh, muj
        self.y = self.R.T @ (self.x - self.c)
        here = F.sample(self.y)
        self.val = here is not None
        self.d = here[0] - r if self.val else np.inf
        self.m = self.R @ here[1] if self.val else np.zeros(3)
        self.W = self.R @ here[2] @ self.R.T if self.val else np.zeros((3, 3))
        self.act = self.val and self.d < eps
        self.y0 = self.R0.T @ (self.xp - self.cp)
        prev = F.sample(self.y0)
        self.val0 = prev is not None
        self.d0 = prev[0] - r if self.val0 else np.inf
        q0 = self.R0 @ prev[1] if self.val0 else np.zeros(3)
        self.s0 = float(np.sqrt(q0 @ q0))
        self.fric = self.val0 and self.s0 >= TINY
        self.n0 = q0 / self.s0 if self.fric else np.zeros(3)
        self.W0 = self.R0 @ prev[2] @ self.R0.T if self.fric else np.zeros((3, 3))
        self.pen = max(0.0, eps - self.d0) if self.fric else 0.0
        self.lam = muj * k * self.pen
        self.act0 = self.fric and self.d0 < eps
        self.P0 = I3 - np.outer(self.n0, self.n0)
        self.D = (self.x - self.c) - self.R @ self.y0
        self.w = self.P0 @ self.D
        self.r_w = float(np.sqrt(self.w @ self.w))
        self.a1 = f1(self.r_w, eh)
        self.f2r = f2(self.r_w, eh) / self.r_w if self.r_w > 1e-9 else 0.0
        self.phi1 = k * (self.d - eps) if self.act else 0.0

    def E(self):
        return (0.5 * self.k * (self.d - self.eps) ** 2 if self.act else 0.0) + self.lam * f0(self.r_w, self.eh)

    def gn(self):
        return self.phi1 * self.m

    def g(self):
        return self.gn() + self.lam * self.a1 * self.w

    def curvature(self):
        """the part of H_n that the projected modes leave out"""
        return self.phi1 * self.W if self.act and self.drop != "curv" else np.zeros((3, 3))

    def Hn(self, exact=True):
        if not self.act:
            return np.zeros((3, 3))
        H = self.k * np.outer(self.m, self.m)
        return H + self.curvature() if exact else H

    def M(self):
        return self.a1 * self.P0 + self.f2r * np.outer(self.w, self.w)

    def B(self):
        return self.a1 * I3 + self.f2r * np.outer(self.w, self.w)

    def Jn(self):
        """d(a1 w)/d(n0)"""
        return -self.B() @ (float(self.n0 @ self.D) * I3 + np.outer(self.n0, self.D))

    def dn0_dxp(self):
        """n0 = R0 grad phi(y0) / s0 turns with y0 through Hess phi(y0)"""
        return np.zeros((3, 3)) if self.drop == "hess0" or not self.fric else self.P0 @ self.W0 / self.s0

    # ---- derivatives of g
    def dg_dc(self):
        return -self.Hn() - self.lam * self.M()

    def dg_dth(self):
        return self.Hn() @ skew(self.x - self.c) - skew(self.gn()) + self.lam * self.M() @ skew(self.R @ self.y0)

    def lagged(self, dd0, dn0, dD):
        """dd0 (3): d(d0)/d(parameter); dn0 (3 x 3): d(n0)/d(parameter); dD (3 x 3): d(D)/d(parameter)"""
        if not self.fric:
            return np.zeros((3, 3))
        out = np.zeros((3, 3))
        if self.act0:
            out -= self.mu * self.k * np.outer(self.a1 * self.w, dd0)
        return out + self.lam * (self.M() @ dD + self.Jn() @ dn0)

    def dg_dxp(self):
        # y0 moves by R0^T dx_prev: d0 by s0 n0, D by -R R0^T
        return self.lagged(self.s0 * self.n0, self.dn0_dxp(), -self.R @ self.R0.T)

    def dg_dcp(self):
        return -self.dg_dxp()

    def dg_dthp(self):
        if not self.fric:
            return np.zeros((3, 3))
        arm = skew(self.xp - self.cp)
        # y0 turns as if x_prev moved by arm dtheta; n0 turns with the field on top of that
        return self.lagged(self.s0 * self.n0 @ arm, self.dn0_dxp() @ arm - skew(self.n0), -self.R @ self.R0.T @ arm)

    def dr(self):
        return (-self.k * self.m if self.act else np.zeros(3)) + (self.mu * self.k * self.a1 * self.w if self.act0 else np.zeros(3))

    def dmu(self):
        return self.k * self.pen * self.a1 * self.w


def pairs(x, xp, F, c, R, cp, R0, r, mu, mask, k, eps, eh, drop=None):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    xp = np.asarray(xp, np.float64).reshape(-1, 3)
    for v in range(len(x)):
        for j in range(len(F)):
            if (int(mask[v]) >> j) & 1:
                yield v, j, Pair(x[v], xp[v], F[j], c[j], R[j], cp[j], R0[j], r[j], mu[j], k, eps, eh, drop)


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


def force(x, xp, F, c, *rest):
    """(n, 6): -sum_v g_v of every field and -sum_v (x_v - c) x g_v about its centre (frozen dofs not masked)"""
    xs = np.asarray(x, np.float64).reshape(-1, 3)
    out = np.zeros((len(F), 6))
    for v, j, P in pairs(x, xp, F, c, *rest):
        g = P.g()
        out[j, 0:3] -= g
        out[j, 3:6] -= np.cross(xs[v] - c[j], g)
    return out


def _free(frozen, p):
    free = (np.asarray(frozen).reshape(-1, 3) == 0).astype(np.float64)
    return free, np.asarray(p, np.float64).reshape(-1, 3) * free


def backprop_prev(x, xp, p, frozen, *A, **kw):
    """(NV, 3): what a reverse step adds to pos_grad[s-1]: X = -(dg/dx_prev)^T p_v on the free dofs, p's frozen dofs not counting"""
    free, p = _free(frozen, p)
    out = np.zeros_like(p)
    for v, j, P in pairs(x, xp, *A, **kw):
        out[v] -= P.dg_dxp().T @ p[v]
    return out * free


def sdf_grad(x, xp, p, frozen, *A, **kw):
    """(n, 14): the shares of one reverse step in d(loss)/d(c_j, theta_j, cp_j, theta_p_j, mu_j, r_j)"""
    free, p = _free(frozen, p)
    G = np.zeros((len(A[0]), 14))
    for v, j, P in pairs(x, xp, *A, **kw):
        G[j, 0:3] -= P.dg_dc().T @ p[v]
        G[j, 3:6] -= P.dg_dth().T @ p[v]
        G[j, 6:9] -= P.dg_dcp().T @ p[v]
        G[j, 9:12] -= P.dg_dthp().T @ p[v]
        G[j, 12] -= float(p[v] @ P.dmu())
        G[j, 13] -= float(p[v] @ P.dr())
    return G


def active_sets(x, xp, *A):
    """(NV, n) boolean arrays over the masked pairs: y valid, y0 valid, d < eps, d0 < eps (with friction possible)"""
    NV, n = _nv(x), len(A[0])
    val, val0, act, act0 = (np.zeros((NV, n), bool) for _ in range(4))
    for v, j, P in pairs(x, xp, *A):
        val[v, j], val0[v, j], act[v, j], act0[v, j] = P.val, P.val0, P.act, P.act0
    return val, val0, act, act0


def flat(fields):
    """what tsl_set_sdfs takes: (samples one field after the other, dims (n, 3) int32, origins (n, 3), spacings (n))"""
    return (np.concatenate([f.s.reshape(-1) for f in fields]), np.array([f.dims for f in fields], np.int32),
            np.array([f.o for f in fields]), np.array([f.h for f in fields]))
