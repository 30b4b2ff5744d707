"""The wind restated in dense NumPy, loops over faces, no cleverness: what csrc/k_wind.hpp has to compute.

A wind list is (faces (n, 3) corner vertices, w (n) weights); x, xp (NV, 3) the positions and the start-of-step positions; W (3) the wind velocity;
cn, ct the normal and the tangential drag coefficient; dt the step.

    a = 1/2 (xp_1 - xp_0) x (xp_2 - xp_0), A0 = |a|,  M = w [ct A0 I + (cn - ct) a a^T / A0],  r = (xbar - xpbar) / dt - W,
    E = dt / 2 sum_f r^T M r,  g_a = M r / 3,  H_ab = M / (9 dt);  a face with A0 < 1e-12 contributes nothing.
"""
import numpy as np

AREA_MIN = 1e-12


class Face:
    """one wind face at the state (x, xp): a, A0, ok, M, r, the corners"""

    def __init__(self, v, w, x, xp, W, cn, ct, dt):
        self.v = [int(q) for q in v]
        self.w = w
        p0, p1, p2 = (xp[q] for q in self.v)
        self.e1, self.e2 = p1 - p0, p2 - p0
        self.a = 0.5 * np.cross(self.e1, self.e2)
        self.A0 = np.sqrt(self.a @ self.a)
        self.ok = bool(self.A0 >= AREA_MIN)
        self.r = (x[self.v].sum(axis=0) / 3.0 - xp[self.v].sum(axis=0) / 3.0) / dt - np.asarray(W, np.float64)
        self.cn, self.ct, self.dt = cn, ct, dt
        self.M = w * (ct * self.A0 * np.eye(3) + (cn - ct) * np.outer(self.a, self.a) / self.A0) if self.ok else np.zeros((3, 3))


def faces_of(faces, w, x, xp, W, cn, ct, dt):
    return [Face(faces[i], w[i], x, xp, W, cn, ct, dt) for i in range(len(faces))]


def energy(x, xp, faces, w, W, cn, ct, dt):
    e = 0.0
    for f in faces_of(faces, w, x, xp, W, cn, ct, dt):
        e += 0.5 * dt * (f.r @ f.M @ f.r)
    return e


def gradient(x, xp, faces, w, W, cn, ct, dt):
    """(NV, 3), unmasked"""
    g = np.zeros_like(x)
    for f in faces_of(faces, w, x, xp, W, cn, ct, dt):
        for v in f.v:
            g[v] += f.M @ f.r / 3.0
    return g


def hessian(x, xp, faces, w, W, cn, ct, dt):
    """dense (3 NV, 3 NV), unmasked"""
    NV = len(x)
    H = np.zeros((3 * NV, 3 * NV))
    for f in faces_of(faces, w, x, xp, W, cn, ct, dt):
        for va in f.v:
            for vb in f.v:
                H[3 * va:3 * va + 3, 3 * vb:3 * vb + 3] += f.M / (9.0 * dt)
    return H


def _free_p(p, frozen):
    return np.asarray(p, np.float64) * (np.asarray(frozen) == 0)


def backprop_prev(x, xp, p, frozen, faces, w, W, cn, ct, dt, with_a=True):
    """(NV, 3): -(dg / dx_prev)^T p on the free dofs, p counted on its free dofs.  with_a False: the derivative through the lagged area vector is
    dropped (a mutation the tests must catch)."""
    pf = _free_p(p, frozen)
    out = np.zeros_like(x)
    for f in faces_of(faces, w, x, xp, W, cn, ct, dt):
        if not f.ok:
            continue
        P = pf[f.v].sum(axis=0)
        thr = f.M @ P / (9.0 * dt)
        c = [thr.copy(), thr.copy(), thr.copy()]
        if with_a:
            a, A0, r = f.a, f.A0, f.r
            q = f.w / 3.0 * (ct * (P @ r) * a / A0 + (cn - ct) * (((a @ r) * P + (a @ P) * r) / A0 - (a @ P) * (a @ r) * a / A0 ** 3))
            t1 = -0.5 * np.cross(f.e2, q)
            t2 = -0.5 * np.cross(q, f.e1)
            c[1] += t1; c[2] += t2; c[0] -= t1 + t2
        for k, v in enumerate(f.v):
            out[v] += c[k]
    return out * (np.asarray(frozen) == 0)


def wind_force(x, xp, faces, w, W, cn, ct, dt):
    """(3,): -sum_f M_f r_f, the net force the wind applies to the cloth (frozen dofs not masked)"""
    s = np.zeros(3)
    for f in faces_of(faces, w, x, xp, W, cn, ct, dt):
        s -= f.M @ f.r
    return s


def wind_grad(x, xp, p, frozen, faces, w, W, cn, ct, dt):
    """(5,): -sum (dg/d.)^T p over the free dofs for W (3), cn, ct"""
    pf = _free_p(p, frozen)
    s = np.zeros(5)
    for f in faces_of(faces, w, x, xp, W, cn, ct, dt):
        if not f.ok:
            continue
        P = pf[f.v].sum(axis=0)
        n0 = f.a / f.A0
        s[0:3] += f.M @ P / 3.0
        s[3] -= f.w * f.A0 * (n0 @ f.r) * (n0 @ P) / 3.0
        s[4] -= f.w * f.A0 * (f.r @ P - (n0 @ f.r) * (n0 @ P)) / 3.0
    return s


# ---- the gather lists of csrc/handle_host.hpp for a face list, restated (corner vertices cv (n, 3); block addresses left to the caller)
def gather_lists(cv):
    cv = np.asarray(cv).reshape(-1, 3)
    ve = sorted((int(cv[i, a]), 3 * i + a) for i in range(len(cv)) for a in range(3))
    be = sorted(((int(cv[i, a]), int(cv[i, b])), 9 * i + 3 * a + b) for i in range(len(cv)) for a in range(3) for b in range(3))
    vl_v, vl_ptr, bl_key, bl_ptr = [], [], [], []
    for q, (v, _) in enumerate(ve):
        if q == 0 or v != ve[q - 1][0]:
            vl_v.append(v); vl_ptr.append(q)
    vl_ptr.append(len(ve))
    for q, (k, _) in enumerate(be):
        if q == 0 or k != be[q - 1][0]:
            bl_key.append(k); bl_ptr.append(q)
    bl_ptr.append(len(be))
    return dict(vl_v=vl_v, vl_ptr=vl_ptr, vl_ent=[e for _, e in ve], bl_key=bl_key, bl_ptr=bl_ptr, bl_ent=[e for _, e in be])
