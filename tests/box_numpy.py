"""Dense NumPy restatement of the rounded-box colliders (csrc/k_box.hpp, csrc/box_host.hpp) for tests/test_box_numpy.py and
tests/test_gpu_boxes.py.

Box j: centre c_j, rotation matrix R_j (columns u_i: the box axes in the world), previous pose cp_j, R0_j (where the box was at the start of the
step), half extents h_j >= 0, rounding radius r_j > 0, friction mu_j; shared stiffness k, shell eps, friction regularisation eh = eps_v dt.  For
vertex v with position x and start-of-step position x_prev:
  y  = R^T (x - c),        b  = clamp(y, -h, h),    free_i  = [-h_i < y_i < h_i]
  q  = R (y - b),  rho = |q|,  n = q / rho,  d = rho - r
  y0 = R0^T (x_prev - cp), b0 = clamp(y0, -h, h),   free0_i = [-h_i < y0_i < h_i]
  q0 = R0 (y0 - b0), rho0, n0, d0 = rho0 - r
  lam = mu k max(0, eps - d0),  dc = (c + R b0) - (cp + R0 b0),  D = (x - x_prev) - dc,  P0 = I - n0 n0^T,  w = P0 D,  r_w = |w|,  a1 = f1(r_w)
  E = [d < eps] 1/2 k (d - eps)^2 + lam f0(r_w),  g = [d < eps] k (d - eps) n + lam a1 w
  H = H_n + lam M,  H_n = [d < eps] (k n n^T + k (d - eps) / rho (I - n n^T - sum_i free_i u_i u_i^T)),  M = a1 P0 + [r_w > 1e-9] (f2 / r_w) w w^T
The projected operator drops the second part of H_n.  A pair with rho < 1e-12 contributes nothing; one with rho0 < 1e-12 has no friction.
Everything here is written from these formulas with dense matrices and loops, not from the kernels; the gap is formed in extended precision.  The
derivatives are the dense Jacobians dg/d(parameter); a rotation parameter is a world-frame rotation vector applied on the left, R <- exp([theta]x) R.
The keyword `drop` takes one term out of the derivatives, for the sensitivity figures: "free" (sum free u u^T in H_n), "delta" (Delta in the lagged
columns), "spin_n0" (the turn of n0 with the previous pose), "arm" (the (R b0) x . term of d/dtheta)."""
import numpy as np

from collider_numpy import f0, f1, f2   # the friction regularisation of k_contact.hpp, restated there

I3 = np.eye(3)
TINY = 1e-12
LD = np.longdouble


def skew(a):
    """[a]x: skew(a) @ b = a x b"""
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def quat_to_R(q):
    """the rotation matrix of q / |q|, q = (s, x, y, z): the formula of engine/gripper_single.quat_to_rotmat, the norm added in the library's order"""
    q = np.asarray(q, np.float64)
    s, x, y, z = (q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])).tolist()
    return np.array([[s * s + x * x - y * y - z * z, 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), s * s - x * x + y * y - z * z, 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), s * s - x * x - y * y + z * z]])


def rot(theta):
    """exp([theta]x) (Rodrigues)"""
    theta = np.asarray(theta, np.float64)
    a = float(np.linalg.norm(theta))
    if a < 1e-300:
        return I3.copy()
    K = skew(theta / a)
    return I3 + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def full_mask(NV, n_box):
    return np.full(NV, (1 << n_box) - 1, np.uint8)


def mask_from_ids(NV, ids_per_box):
    m = np.zeros(NV, np.uint8)
    for j, ids in enumerate(ids_per_box):
        m[np.asarray(ids, np.int64)] |= np.uint8(1 << j)
    return m


def _closest(xv, c, R, h, r):
    """(y, b, free, q, |q|, |q| - r) in extended precision, rounded once at the end"""
    x, cc, RR, hh = np.asarray(xv, LD), np.asarray(c, LD), np.asarray(R, LD), np.asarray(h, LD)
    y = RR.T @ (x - cc)
    b = np.minimum(np.maximum(y, -hh), hh)
    free = (y > -hh) & (y < hh)
    q = RR @ (y - b)
    rho = np.sqrt((q * q).sum())
    return y.astype(np.float64), b.astype(np.float64), free, q.astype(np.float64), float(rho), float(rho - LD(r))


class Pair:
    """the quantities of one (vertex, box) pair; ok False: rho < 1e-12, the pair contributes nothing"""

    def __init__(self, xv, xpv, c, R, cp, R0, h, r, muj, k, eps, eh, drop=None):
        self.drop = drop
        self.x, self.xp, self.c, self.R, self.cp, self.R0 = (np.asarray(a, np.float64) for a in (xv, xpv, c, R, cp, R0))
        self.y, self.b, self.free, q, self.rho, self.d = _closest(xv, c, R, h, r)
        self.ok = self.rho >= TINY
        if not self.ok:
            return
        self.n = q / self.rho
        self.y0, self.b0, self.free0, self.q0, self.rho0, self.d0 = _closest(xpv, cp, R0, h, r)
        self.fric = self.rho0 >= TINY
        self.n0 = self.q0 / self.rho0 if self.fric else np.zeros(3)
        self.pen = max(0.0, eps - self.d0) if self.fric else 0.0
        self.lam = muj * k * self.pen
        self.P0 = I3 - np.outer(self.n0, self.n0)
        self.dc = (self.c + self.R @ self.b0) - (self.cp + self.R0 @ self.b0)
        self.D = (self.x - self.xp) - self.dc
        self.w = self.P0 @ self.D
        self.r_w = float(np.sqrt(self.w @ self.w))
        self.a1 = f1(self.r_w, eh)
        self.f2r = f2(self.r_w, eh) / self.r_w if self.r_w > 1e-9 else 0.0
        self.k, self.eps, self.eh, self.mu = k, eps, eh, muj
        self.act = self.d < eps
        self.act0 = self.fric and self.d0 < eps
        self.phi1 = k * (self.d - eps) if self.act else 0.0
        self.U = sum((np.outer(self.R[:, i], self.R[:, i]) for i in range(3) if self.free[i]), np.zeros((3, 3)))
        self.U0 = sum((np.outer(self.R0[:, i], self.R0[:, i]) for i in range(3) if self.free0[i]), np.zeros((3, 3)))
        self.Delta = sum((np.outer(self.R[:, i] - self.R0[:, i], self.R0[:, i]) for i in range(3) if self.free0[i]), np.zeros((3, 3)))

    def region(self):
        """(number of free axes at x, at x_prev): 2 face, 1 edge, 0 corner (3: inside the core box)"""
        return int(self.free.sum()), int(self.free0.sum())

    def E(self):
        return (0.5 * self.k * (self.d - self.eps) ** 2 if self.act else 0.0) + self.lam * f0(self.r_w, self.eh)

    def gn(self):
        return self.phi1 * self.n

    def g(self):
        return self.gn() + self.lam * self.a1 * self.w

    def curvature(self):
        """the part of H_n that the projected modes leave out"""
        if not self.act:
            return np.zeros((3, 3))
        G = I3 - np.outer(self.n, self.n)
        if self.drop != "free":
            G = G - self.U
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

    def Jn(self):
        return -self.B() @ (float(self.n0 @ self.D) * I3 + np.outer(self.n0, self.D))

    def G0(self):
        return self.P0 - self.U0

    # ---- derivatives of g
    def dg_dc(self):
        return -self.Hn() - self.lam * self.M()

    def dg_dth(self):
        out = self.Hn() @ skew(self.x - self.c) - skew(self.gn())
        if self.drop != "arm":
            out = out + self.lam * self.M() @ skew(self.R @ self.b0)
        return out

    def lagged(self, dd0, dn0, dD):
        """dd0 (3): d(d0)/d(parameter); dn0 (3 x 3): d(n0)/d(parameter); dD (3 x 3): d(D)/d(parameter), the change of b0 included"""
        if not self.fric:
            return np.zeros((3, 3))
        out = np.zeros((3, 3))
        if self.act0:
            out -= self.mu * self.k * np.outer(self.a1 * self.w, dd0)
        return out + self.lam * (self.M() @ dD + self.Jn() @ dn0)

    def _Delta(self):
        return np.zeros((3, 3)) if self.drop == "delta" else self.Delta

    def dg_dxp(self):
        if not self.fric:
            return np.zeros((3, 3))
        return self.lagged(self.n0, self.G0() / self.rho0, -I3 - self._Delta())

    def dg_dcp(self):
        if not self.fric:
            return np.zeros((3, 3))
        return self.lagged(-self.n0, -self.G0() / self.rho0, I3 + self._Delta())

    def dg_dthp(self):
        if not self.fric:
            return np.zeros((3, 3))
        arm = skew(self.xp - self.cp)
        spin = np.zeros((3, 3)) if self.drop == "spin_n0" else -skew(self.n0)
        # y0 turns as if x_prev moved by arm dtheta; n0 turns with the box on top of that; the material point R0 b0 turns with the box
        return self.lagged(self.n0 @ arm, self.G0() @ arm / self.rho0 + spin, -self._Delta() @ arm - skew(self.R0 @ self.b0))

    def dr(self):
        return (-self.k * self.n if self.act else np.zeros(3)) + (self.mu * self.k * self.a1 * self.w if self.act0 else np.zeros(3))

    def dmu(self):
        return self.k * self.pen * self.a1 * self.w


def pairs(x, xp, c, R, cp, R0, h, r, mu, mask, k, eps, eh, drop=None):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    xp = np.asarray(xp, np.float64).reshape(-1, 3)
    for v in range(len(x)):
        for j in range(len(r)):
            if (int(mask[v]) >> j) & 1:
                P = Pair(x[v], xp[v], c[j], R[j], cp[j], R0[j], h[j], r[j], mu[j], k, eps, eh, drop)
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


def force(x, xp, c, *rest):
    """(n_box, 6): -sum_v g_v of every box and -sum_v (x_v - c) x g_v about its centre (frozen dofs not masked)"""
    xs = np.asarray(x, np.float64).reshape(-1, 3)
    F = np.zeros((len(c), 6))
    for v, j, P in pairs(x, xp, c, *rest):
        g = P.g()
        F[j, 0:3] -= g
        F[j, 3:6] -= np.cross(xs[v] - c[j], g)
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


def box_grad(x, xp, p, frozen, *A, **kw):
    """(n_box, 14): the shares of one reverse step in d(loss)/d(c_j, theta_j, cp_j, theta_p_j, mu_j, r_j)"""
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
    """(NV, n_box) arrays over the masked pairs: d < eps, d0 < eps, the number of free axes at x and at x_prev (9 where the pair is masked out)"""
    NV, n = _nv(x), len(A[5])
    act, act0 = np.zeros((NV, n), bool), np.zeros((NV, n), bool)
    reg, reg0 = np.full((NV, n), 9), np.full((NV, n), 9)
    for v, j, P in pairs(x, xp, *A):
        act[v, j], act0[v, j] = P.act, P.act0
        reg[v, j], reg0[v, j] = P.region()
    return act, act0, reg, reg0


def place(c, R, cp, R0, h, r, k, eps, eh, y0_core, n0_local, d0_off, slip, slip_dir, d_off):
    """One vertex against the box (c, R, cp, R0, h, r).  x_prev: over the point y0_core of the core box's surface (local coordinates), along the local
    unit direction n0_local (zero along the free axes), with gap d0 = eps + d0_off.  x: the box's material point carried along, plus a slip of
    length `slip` in the tangent plane of n0 (slip_dir: angle in that plane), plus the multiple of n0 that makes d = eps + d_off."""
    nl = np.asarray(n0_local, np.float64)
    nl = nl / np.linalg.norm(nl)
    xp = cp + R0 @ (np.asarray(y0_core, np.float64) + (r + eps + d0_off) * nl)
    P = Pair(xp, xp, cp, R0, cp, R0, h, r, 0.0, k, eps, eh)
    n0, b0 = P.n, P.b
    dc = (c + R @ b0) - (cp + R0 @ b0)
    seed = R0[:, int(np.argmin(np.abs(nl)))]
    t1 = seed - n0 * (n0 @ seed)
    t1 = t1 / np.linalg.norm(t1)
    t2 = np.cross(n0, t1)
    base = xp + dc + slip * (np.cos(slip_dir) * t1 + np.sin(slip_dir) * t2)
    gap = lambda al: Pair(base + al * n0, xp, c, R, cp, R0, h, r, 0.0, k, eps, eh).d - (eps + d_off)
    lo, hi = -0.9 * (r + eps + d0_off), 6e-3
    assert gap(lo) < 0 < gap(hi), (gap(lo), gap(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gap(mid) < 0 else (lo, mid)
    return xp, base + 0.5 * (lo + hi) * n0
