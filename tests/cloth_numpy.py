"""Restatement of the spring cloth (csrc/k_cloth.hpp; k_pg_face / k_pg_hinge of csrc/k_param.hpp) for tests/test_cloth_numpy.py and
tests/test_gpu_cloth_elements.py, written from the reference's formulas (engine/model_fold_offset.py, line numbers below), not from the kernels
and not from oracle/tslo_cloth.cpp.  The pattern is that of tests/tet_numpy.py, whose backends and helpers it uses: every function takes a backend
`xp`, MP (mpmath at 50 digits, the reference proper) or F64 (NumPy float64 scalars, the same formulas in the same plain order: it only measures
what double precision delivers, see tet_numpy.bound).  Nothing here calls the GPU except cloth_context().

Conventions restated (l, m = vertex slots of a face, j, k = components):
- normal n = unit((b - a) x (c - b)) (:169-174); dihedral of faces i1, i2 over slot l (:126-138): c = n1 . n2, theta = acos(c) where c < 0.999999, else
  2 sqrt|1 - c| / sqrt(1 + c); theta is negated where n2 . e < -1e-10 |e|, e = x[f2v[i1][(l + 1) % 2]] - x[f2v[i1][l]] (the engine's documented
  form of the reference's `< 0`: values within 1e-10 |e| of zero count as zero);
- face energy (:149-167): Kl (1 - len / li)^2 li per spring (slot l to slot l + 1, rest length li[l]) + Ka (1 - A / V)^2 V; gradient (:653-677);
- spring block (:472-522): K = dl G + dl2 d d^T with the reference's G: G_jj = (len^2 - delta_j^2) / len^3, G_jk = + delta_j delta_k / len^3 -- the
  derivative of d has a minus there; `literal=False` takes the minus (for the difference test only);
- area block (:526-580): darea2 g_l g_m^T + darea D, D the four second-derivative formulas (:296-377) in the shorthand C(a, b) = (p2 - p1)_a (p3 - p1)_b
  - (p3 - p1)_a (p2 - p1)_b, e = p2 - p3, w = p3 - p1, T = 2 A; compute_area_dxy_p12 doubles one term (:369): `literal=False` takes it once;
- second-order bending part of a face (:415-448, :585-614): mat_M, mat_N, angle, heights, c_i, d_i per slot, and the block that reads c_i[l][.] and
  mat_N[l * 3 + .] with l the vertex slot, that is faces 0..2 of the cloth (zero where the cloth has fewer faces, as the engine documents it);
  the tables come from the host mirror's init_mesh, wrongly filled slots included (slot 0 of the first triangle of an odd cell is never
  written and names face 0; its slot 2 is overwritten);
- hinges (counter_face > own face): energy (:108-120), the four vertex gradients (:379-402), Gauss-Newton block d2 g g^T (:616-637);
- projection: spd 1 eigen-clamps every 3 x 3 spring block, spd 2 the whole 9 x 9 face block on top;
- update_ref_angle (:176-185); d gradient / d Kl, Ka, Kb = the gradient terms with that constant at 1;
- frozen rule as in tet_numpy (rows and columns removed, diagonal m / dt^2, gradient entries zero).

Every decision (sign test, series switch, `en` flip, plastic threshold) is recorded with a normalised distance from its threshold; decisions_safe()
asserts that each is either zero by construction or at least 1e-6 away, in both backends."""
import functools

import mpmath as mp
import numpy as np

from tet_numpy import F64, MP, R1, R2, U, bound, fro  # noqa: F401

COS_SWITCH = 0.999999
SIGN_TOL = 1e-10
MASS, DT = 1e-30, 5e-3
MDT2 = MASS / DT ** 2
SAFE = 1e-6


# ------------------------------------------------------------------------------------------------ three-vectors on lists
def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(xp, a):
    return xp.sqrt(_dot(a, a))


def _scal(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def _unit(xp, a):
    n = _norm(xp, a)
    return [a[0] / n, a[1] / n, a[2] / n]


def _neg(a):
    return [-a[0], -a[1], -a[2]]


def _z(xp, *shape):
    if len(shape) == 1:
        return [xp.num(0) for _ in range(shape[0])]
    return [_z(xp, *shape[1:]) for _ in range(shape[0])]


# ------------------------------------------------------------------------------------------------ tables
class ClothTables:
    """one cloth: index tables and rest data of the host mirror's init_mesh, constants, v_offset"""
    def __init__(self, N, M, dx, Kl=1000.0, Ka=1000.0, Kb=100.0, k_angle=3.14, v_offset=0):
        from thinshelllab_amd.engine.model_fold_offset import Cloth
        c = Cloth(N, DT, dx * N, 0, 40.0, v_offset, is_square=False, M=M)
        c.init_mesh()
        c._rest()
        d = c._desc()
        d.update(Kl=float(Kl), Ka=float(Ka), Kb=float(Kb), k_angle=float(k_angle), mass=MASS)
        self.desc = d
        self.N, self.M, self.NV, self.NF, self.dx, self.v_offset = N, M, d["NV"], d["NF"], float(d["dx"]), v_offset
        self.Kl, self.Ka, self.Kb, self.k_angle = d["Kl"], d["Ka"], d["Kb"], d["k_angle"]
        self.f2v, self.cf, self.cp = d["f2v"].astype(int), d["counter_face"].astype(int), d["counter_point"].astype(int)
        self.V, self.li = np.asarray(d["rest_area"], float), np.asarray(d["rest_len"], float).reshape(-1, 3)
        self.hinges = [(f, l) for f in range(self.NF) for l in range(3) if self.cf[f, l] > f]

    def hinge_verts(self, f, l):
        """(local vertices of the stencil, i2, p4, p21, p22) of compute_bending_grad (:379-389)"""
        i2, p4 = self.cf[f, l], self.cp[f, l]
        p21 = (p4 + 1) % 3
        if self.f2v[f, (l + 1) % 3] != self.f2v[i2, p21]:
            p21 = (p4 + 2) % 3
        return [self.f2v[f, l], self.f2v[f, (l + 1) % 3], self.f2v[f, (l + 2) % 3], self.f2v[i2, p4]], i2, p4, p21, 3 - p21 - p4


# ------------------------------------------------------------------------------------------------ angles and decisions
def normals(xp, c, X):
    out = []
    for f in range(c.NF):
        a, b, cc = X[c.f2v[f, 0]], X[c.f2v[f, 1]], X[c.f2v[f, 2]]
        out.append(_unit(xp, _cross(_sub(b, a), _sub(cc, b))))
    return out


def sign_negative(xp, c, X, nrm, i1, i2, l, dec):
    """n2 . e < -1e-10 |e|; the decision quantity is n2 . e / |e|"""
    e = _sub(X[c.f2v[i1, (l + 1) % 2]], X[c.f2v[i1, l]])
    q, ne = _dot(nrm[i2], e), _norm(xp, e)
    if dec is not None:
        dec.append(("sign", i1, l, i2, q / ne + xp.num(SIGN_TOL)))
    return q < -xp.num(SIGN_TOL) * ne


def compute_angle(xp, c, X, nrm, i1, i2, l, dec=None, cos_ulps=(0, ())):
    """cos_ulps = (k, pairs), float64 only: the cosine of the face pairs (i1, i2) in `pairs` moved by k ulps before it is used.  Reference passes the
    pairs that are coplanar by the state's construction: there c = 1 up to rounding, an ulp of c is 1e-8 rad, and no float64 evaluation
    determines n1 . n2 better than to an ulp"""
    cos = _dot(nrm[i1], nrm[i2])
    if cos_ulps[0] and (i1, i2) in cos_ulps[1]:
        for _ in range(abs(cos_ulps[0])):
            cos = np.nextafter(cos, np.inf if cos_ulps[0] > 0 else -np.inf)
    if dec is not None:
        dec.append(("switch", i1, l, i2, (1 - cos) / (1 - xp.num(COS_SWITCH)) - 1))
    if cos < xp.num(COS_SWITCH):
        theta = xp.acos(cos)
    else:
        theta = 2 * xp.sqrt(abs(1 - cos)) / xp.sqrt(1 + cos)
    if sign_negative(xp, c, X, nrm, i1, i2, l, dec):
        theta = -theta
    return theta


# ------------------------------------------------------------------------------------------------ membrane of one face
def face_energy(xp, P, li, V, Kl, Ka):
    eS = xp.num(0)
    for l in range(3):
        ln = _norm(xp, _sub(P[(l + 1) % 3], P[l]))
        base = xp.num(li[l])
        eS = eS + Kl * (1 - ln / base) ** 2 * base
    area = _norm(xp, _cross(_sub(P[1], P[0]), _sub(P[2], P[0]))) * xp.num(0.5)
    V = xp.num(V)
    return eS, Ka * (1 - area / V) ** 2 * V


def spring_grad(xp, P, li, Kl):
    g = _z(xp, 3, 3)
    for l in range(3):
        m = (l + 1) % 3
        delta = _sub(P[l], P[m])
        ln = _norm(xp, delta)
        dl = -Kl * 2 * (1 - ln / xp.num(li[l]))
        for j in range(3):
            t = delta[j] * dl / ln
            g[l][j] = g[l][j] + t
            g[m][j] = g[m][j] - t
    return g


class _Tri:
    """the shorthand of the area derivatives for one ordering (p1, p2, p3) of a face's vertices"""
    def __init__(self, p1, p2, p3, T):
        self.e, self.w, self.T = _sub(p2, p3), _sub(p3, p1), T
        u = _sub(p2, p1)
        self.C = [[None] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(3):
                if a != b:
                    self.C[a][b] = u[a] * self.w[b] - self.w[a] * u[b]

    def S(self, dim, d1, d2):
        return self.e[d1] * self.C[dim][d1] + self.e[d2] * self.C[dim][d2]

    def dx(self, dim):                       # compute_area_dx (:312-325): dA/dp1[dim] = S / (2 T)
        d1 = 1 if dim == 0 else 0
        return self.S(dim, d1, 3 - d1 - dim) / self.T / 2

    def dx2(self, dim):                      # :296-310
        d1 = 1 if dim == 0 else 0
        d2 = 3 - d1 - dim
        return ((self.e[d1] ** 2 + self.e[d2] ** 2) / self.T - self.S(dim, d1, d2) ** 2 / self.T ** 3) / 2

    def dxy_p1(self, dim, d1):               # :327-341
        d2 = 3 - d1 - dim
        return ((-self.e[dim]) * self.e[d1] / self.T
                - ((-self.e[dim]) * self.C[dim][d1] + self.e[d2] * self.C[d1][d2]) * self.S(dim, d1, d2) / self.T ** 3) / 2

    def dx2_p12(self, dim):                  # :343-361
        d1 = 1 if dim == 0 else 0
        d2 = 3 - d1 - dim
        return ((self.w[d1] * self.e[d1] + self.w[d2] * self.e[d2]) / self.T
                - self.S(dim, d1, d2) * (self.w[d1] * self.C[dim][d1] + self.w[d2] * self.C[dim][d2]) / self.T ** 3) / 2

    def dxy_p12(self, dim, d1, slip):        # :363-377, slip = 2 as the reference has it
        d2 = 3 - d1 - dim
        return ((self.C[dim][d1] + (-self.w[dim]) * self.e[d1]) / self.T
                - (slip * (-self.w[dim]) * self.C[dim][d1] + self.w[d2] * self.C[d1][d2]) * self.S(dim, d1, d2) / self.T ** 3) / 2


def _area2(xp, P):
    return _norm(xp, _cross(_sub(P[1], P[0]), _sub(P[2], P[0])))


def area_grad(xp, P, V, Ka):
    T = _area2(xp, P)
    da = -Ka * 2 * (1 - T * xp.num(0.5) / xp.num(V))
    return [[da * _Tri(P[l], P[(l + 1) % 3], P[(l + 2) % 3], T).dx(j) for j in range(3)] for l in range(3)]


def spring_blocks(xp, P, li, Kl, literal=True):
    """the three 3 x 3 blocks H_me of a face (:472-499)"""
    out = []
    for l in range(3):
        delta = _sub(P[l], P[(l + 1) % 3])
        ln = _norm(xp, delta)
        d = [delta[j] / ln for j in range(3)]
        base = xp.num(li[l])
        dl, dl2 = -Kl * 2 * (1 - ln / base), Kl * 2 / base
        K = _z(xp, 3, 3)
        for j in range(3):
            for k in range(3):
                if j == k:
                    G = (ln ** 2 - delta[j] ** 2) / ln ** 3
                else:
                    G = delta[j] * delta[k] / ln ** 3
                    if not literal:
                        G = -G
                K[j][k] = dl * G + dl2 * d[j] * d[k]
        out.append(K)
    return out


def clamp3(xp, K):
    """eigen-clamp of a 3 x 3 spring block (symmetric as built)"""
    w, V = xp.eigh([[(K[i][j] + K[j][i]) / 2 for j in range(3)] for i in range(3)])
    out = _z(xp, 3, 3)
    for i in range(3):
        for j in range(3):
            s = xp.num(0)
            for e in range(3):
                if w[e] > 0:
                    s = s + w[e] * V[i][e] * V[j][e]
            out[i][j] = s
    return out


def scatter_springs(xp, K3):
    """:511-522: + on the two diagonal vertex blocks of a spring, - off them; index [(l, j)][(m, k)] = [3 l + j][3 m + k]"""
    L = _z(xp, 9, 9)
    for l in range(3):
        m = (l + 1) % 3
        for j in range(3):
            for k in range(3):
                v = K3[l][j][k]
                L[3 * l + j][3 * l + k] = L[3 * l + j][3 * l + k] + v
                L[3 * l + j][3 * m + k] = L[3 * l + j][3 * m + k] - v
                L[3 * m + j][3 * l + k] = L[3 * m + j][3 * l + k] - v
                L[3 * m + j][3 * m + k] = L[3 * m + j][3 * m + k] + v
    return L


def area_block(xp, P, V, Ka, literal=True):
    T = _area2(xp, P)
    V = xp.num(V)
    da, da2 = -Ka * 2 * (1 - T * xp.num(0.5) / V), Ka * 2 / V
    slip = 2 if literal else 1
    cyc = [_Tri(P[l], P[(l + 1) % 3], P[(l + 2) % 3], T) for l in range(3)]
    fd = [[cyc[l].dx(j) for j in range(3)] for l in range(3)]
    L = _z(xp, 9, 9)
    for l in range(3):
        for m in range(3):
            t = cyc[l] if l == m else _Tri(P[l], P[m], P[3 - l - m], T)
            for j in range(3):
                for k in range(3):
                    if j == k:
                        D = t.dx2(j) if l == m else t.dx2_p12(j)
                    else:
                        D = t.dxy_p1(j, k) if l == m else t.dxy_p12(j, k, slip)
                    L[3 * l + j][3 * m + k] = fd[l][j] * fd[m][k] * da2 + da * D
    return L


# ------------------------------------------------------------------------------------------------ bending
def prepare_bending(xp, c, X, nrm, ra, dec=None, cos_ulps=(0, ())):
    """prepare_bending (:415-448): per face dict(M, N, angle, h, ci, di), lists over the three slots"""
    Kb, dx = xp.num(c.Kb), xp.num(c.dx)
    out = []
    for i in range(c.NF):
        Mm, Nm, ang, hgt, ci = [], [], [], [], []
        for l in range(3):
            p, a, b = X[c.f2v[i, l]], X[c.f2v[i, (l + 1) % 3]], X[c.f2v[i, (l + 2) % 3]]
            edge = _sub(b, a)
            nb = c.cf[i, l]
            theta, judge = None, True
            if nb != -1:
                theta = compute_angle(xp, c, X, nrm, i, nb, l, dec, cos_ulps)
                judge = not sign_negative(xp, c, X, nrm, i, nb, l, None)
            nd = _neg(nrm[i]) if judge else nrm[i]
            en = _cross(nd, edge)
            ap = _sub(a, p)
            s = _dot(en, ap)
            if dec is not None:
                dec.append(("en", i, l, nb, s / (_norm(xp, en) * _norm(xp, ap))))
            if s > 0:
                en = _neg(en)
            M = [[nd[r] * en[q] for q in range(3)] for r in range(3)]
            ne = _norm(xp, edge)
            Mm.append(M)
            Nm.append([[M[r][q] / ne for q in range(3)] for r in range(3)])
            ang.append(_dot(_unit(xp, ap), _unit(xp, _sub(b, p))))
            hgt.append(abs(_dot(_sub(p, a), en)) / _norm(xp, en))
            ci.append(2 * Kb * (theta - xp.num(ra[i][l])) * dx ** 2 / 3 if nb != -1 else xp.num(0))
        di = [ci[(l + 1) % 3] * ang[(l + 2) % 3] + ci[(l + 2) % 3] * ang[(l + 1) % 3] - ci[l] for l in range(3)]
        out.append(dict(M=Mm, N=Nm, angle=ang, h=hgt, ci=ci, di=di))
    return out


def bending_block(xp, c, prep, i):
    """the second-order part (:585-614), with c_i[l][.] and mat_N[l * 3 + .] read at face l of the cloth"""
    q = prep[i]
    L = _z(xp, 9, 9)
    for l in range(3):
        for lm in (l, l + 1):
            m = lm % 3
            inv = 1 / (q["h"][l] * q["h"][m])
            H = [[inv * (q["di"][l] * q["M"][m][k][j] + q["di"][m] * q["M"][l][j][k]) for k in range(3)] for j in range(3)]
            if l < c.NF:
                t = prep[l]
                for j in range(3):
                    for k in range(3):
                        if l == m:
                            i1, i2 = (l + 1) % 3, (l + 2) % 3
                            H[j][k] = H[j][k] - t["ci"][i1] * t["N"][i1][j][k] - t["ci"][i2] * t["N"][i2][j][k]
                        else:
                            i3 = 3 - l - m
                            H[j][k] = H[j][k] + t["ci"][i3] * t["N"][i3][j][k]
            for j in range(3):
                for k in range(3):
                    L[3 * l + j][3 * m + k] = L[3 * l + j][3 * m + k] + H[j][k]
                    if l != m:
                        L[3 * m + j][3 * l + k] = L[3 * m + j][3 * l + k] + H[k][j]
    return L


def hinge(xp, c, X, nrm, prep, ra, f, l, dec=None, cos_ulps=(0, ())):
    """one hinge the engine forms: theta, the four d(theta)/dx (:379-402), energy per unit Kb, d(energy)/d(theta) per unit Kb"""
    _, i2, p4, p21, p22 = c.hinge_verts(f, l)
    p11, p12 = (l + 1) % 3, (l + 2) % 3
    q1, q2 = prep[f], prep[i2]
    n1, n2 = nrm[f], nrm[i2]
    g = [_scal(-1 / q1["h"][l], n1),
         [q1["angle"][p12] / q1["h"][p11] * n1[j] + q2["angle"][p22] / q2["h"][p21] * n2[j] for j in range(3)],
         [q1["angle"][p11] / q1["h"][p12] * n1[j] + q2["angle"][p21] / q2["h"][p22] * n2[j] for j in range(3)],
         _scal(-1 / q2["h"][p4], n2)]
    theta = compute_angle(xp, c, X, nrm, f, i2, l, dec, cos_ulps)
    dis = theta - xp.num(ra[f][l])
    dx = xp.num(c.dx)
    return dict(theta=theta, g=g, e1=dis ** 2 * dx ** 2 / 3, dth1=2 * dis * dx ** 2 / 3, d21=2 * dx ** 2 / 3, dis=dis)


def update_ref(xp, c, theta, ra_fl, dec=None):
    """:181-185 for one hinge: the new reference angle"""
    ra_fl, ka = xp.num(ra_fl), xp.num(c.k_angle)
    dis = theta - ra_fl
    ad = abs(dis)
    if dec is not None:
        dec.append(("plastic", ad / ka - 1))
    return ra_fl + (ad - ka) * dis / ad if ad > ka else ra_fl


# ------------------------------------------------------------------------------------------------ one cloth, all elements
FACE_Q = ("eS", "eA", "gS", "gA", "gS1", "gA1", "K3", "HS", "HA", "HB")
HINGE_Q = ("theta", "eB", "gB", "gB1", "g", "G", "newref")


def evaluate(xp, c, x, ra, literal=True, dec=None, cos_ulps=(0, ())):
    """every element quantity of cloth c at the local positions x (NV, 3) and reference angles ra (NF, 3), as object / float arrays:
    faces: eS, eA (energies), gS, gA (3, 3 gradients), gS1, gA1 (per unit Kl, Ka), K3 (3 spring blocks), HS, HA, HB (spring, area and bending parts
    of the 9 x 9 block, indexed [l, j, m, k]);
    hinges in the order of c.hinges: theta, eB, gB (4, 3 = d(energy)/dx), gB1 (per unit Kb), g (d(theta)/dx), G (the Gauss-Newton block
    [a, j, b, k]), newref"""
    X = [[xp.num(v) for v in row] for row in np.asarray(x, dtype=object)]
    Kl, Ka, Kb = xp.num(c.Kl), xp.num(c.Ka), xp.num(c.Kb)
    one = xp.num(1)
    nrm = normals(xp, c, X)
    prep = prepare_bending(xp, c, X, nrm, ra, dec, cos_ulps)
    F = {q: [] for q in FACE_Q}
    for f in range(c.NF):
        P = [X[v] for v in c.f2v[f]]
        eS, eA = face_energy(xp, P, c.li[f], c.V[f], Kl, Ka)
        F["eS"].append(eS); F["eA"].append(eA)
        F["gS"].append(spring_grad(xp, P, c.li[f], Kl)); F["gA"].append(area_grad(xp, P, c.V[f], Ka))
        F["gS1"].append(spring_grad(xp, P, c.li[f], one)); F["gA1"].append(area_grad(xp, P, c.V[f], one))
        F["K3"].append(spring_blocks(xp, P, c.li[f], Kl, literal))
        F["HS"].append(scatter_springs(xp, F["K3"][-1]))
        F["HA"].append(area_block(xp, P, c.V[f], Ka, literal))
        F["HB"].append(bending_block(xp, c, prep, f))
    Hg = {q: [] for q in HINGE_Q}
    for f, l in c.hinges:
        h = hinge(xp, c, X, nrm, prep, ra, f, l, None, cos_ulps)
        Hg["theta"].append(h["theta"]); Hg["eB"].append(Kb * h["e1"])
        Hg["gB"].append([_scal(Kb * h["dth1"], v) for v in h["g"]]); Hg["gB1"].append([_scal(h["dth1"], v) for v in h["g"]])
        Hg["g"].append(h["g"])
        g12, d2 = [v for w in h["g"] for v in w], Kb * h["d21"]
        Hg["G"].append([[d2 * (a * b) for b in g12] for a in g12])
        Hg["newref"].append(update_ref(xp, c, h["theta"], ra[f][l], dec))
    dt = object if xp is MP else float
    out = {q: np.array(v, dtype=dt) for q, v in F.items()}
    for q in ("HS", "HA", "HB"):
        out[q] = out[q].reshape(c.NF, 3, 3, 3, 3)
    out.update({q: np.array(v, dtype=dt).reshape((len(c.hinges),) + s) for (q, v), s in
                zip(Hg.items(), ((), (), (4, 3), (4, 3), (4, 3), (4, 3, 4, 3), ()))})
    return out


def totals(xp, c, x, ra, what="energy"):
    """energies (E_S, E_A, E_B) of cloth c, or with what = "gradient" their three gradients (NV, 3): the sums of the element terms above without
    the blocks (the difference tests evaluate these many times)"""
    X = [[xp.num(v) for v in row] for row in np.asarray(x, dtype=object)]
    Kl, Ka, Kb = xp.num(c.Kl), xp.num(c.Ka), xp.num(c.Kb)
    nrm = normals(xp, c, X)
    prep = prepare_bending(xp, c, X, nrm, ra)
    if what == "energy":
        E = [xp.num(0)] * 3
        for f in range(c.NF):
            eS, eA = face_energy(xp, [X[v] for v in c.f2v[f]], c.li[f], c.V[f], Kl, Ka)
            E = [E[0] + eS, E[1] + eA, E[2]]
        for f, l in c.hinges:
            E[2] = E[2] + Kb * hinge(xp, c, X, nrm, prep, ra, f, l)["e1"]
        return E
    G = np.array(_z(xp, 3, c.NV, 3), dtype=object)
    for f in range(c.NF):
        P = [X[v] for v in c.f2v[f]]
        gS, gA = spring_grad(xp, P, c.li[f], Kl), area_grad(xp, P, c.V[f], Ka)
        for l in range(3):
            for j in range(3):
                G[0, c.f2v[f, l], j] += gS[l][j]; G[1, c.f2v[f, l], j] += gA[l][j]
    for f, l in c.hinges:
        h = hinge(xp, c, X, nrm, prep, ra, f, l)
        for a, v in enumerate(c.hinge_verts(f, l)[0]):
            for j in range(3):
                G[2, v, j] += Kb * h["dth1"] * h["g"][a][j]
    return G


def ratio(R, q, err, bnd):
    """R.add, and an exact answer where the bound is zero (every float64 evaluation met mp exactly, a sheet flat in z = 0 for instance)"""
    if bnd == 0:
        assert err == 0, (q, err)
    else:
        R.add(q, err, bnd)


# ------------------------------------------------------------------------------------------------ states
class State:
    """cloths (ClothTables), global positions x (nv, 3) in float64, reference angles per cloth; pieces[i][f] = label of the exactly planar piece
    face f of cloth i was built in (-1: none), ruling[i] = None or 0 / 1: the state is a cylinder whose rulings run along grid index j (0: vertices
    of equal i lie on a line parallel to the axis) or i (1)"""
    def __init__(self, name, cloths, x, ra, pieces, ruling):
        self.name, self.cloths, self.x, self.ra, self.pieces, self.ruling = name, cloths, np.asarray(x, float), ra, pieces, ruling
        self.nv = len(self.x)

    def local(self, i, x=None):
        c = self.cloths[i]
        return (self.x if x is None else x)[c.v_offset:c.v_offset + c.NV]

    def __hash__(self):
        return id(self)


def grid(c):
    i, j = np.meshgrid(np.arange(c.N + 1), np.arange(c.M + 1), indexing="ij")
    return i.ravel(), j.ravel()


def _cell_of_face(c, f):
    return (f // 2) // c.M, (f // 2) % c.M


def flat(c, sx=1.0, sy=1.0, shear=0.0):
    i, j = grid(c)
    return np.stack([sx * i * c.dx + shear * j * c.dx, sy * j * c.dx, np.zeros(len(i))], 1), np.zeros(c.NF, int), None


def fold(c, phi, axis=0, line=1):
    """folded by the dihedral phi (signed) about grid line `line` of index i (axis 0) or j (axis 1): both halves exactly planar"""
    i, j = grid(c)
    s, t = (i, j) if axis == 0 else (j, i)
    far = np.maximum(s - line, 0) * c.dx
    u = np.minimum(s, line) * c.dx + far * np.cos(phi)
    z = -far * np.sin(phi)   # (the sign that the reference's convention calls +phi)
    x = np.stack([u, t * c.dx, z], 1) if axis == 0 else np.stack([t * c.dx, u, z], 1)
    cell = np.array([_cell_of_face(c, f)[axis] for f in range(c.NF)])
    return x, (cell >= line).astype(int), axis


def ripple(c, theta, axis=0):
    """zigzag across grid index i (axis 0) or j: strips exactly planar, dihedral +-theta on every grid line between them, edges unstretched"""
    i, j = grid(c)
    s, t = (i, j) if axis == 0 else (j, i)
    u, z = s * c.dx * np.cos(theta / 2), (s % 2) * c.dx * np.sin(theta / 2)
    x = np.stack([u, t * c.dx, z], 1) if axis == 0 else np.stack([t * c.dx, u, z], 1)
    return x, np.array([_cell_of_face(c, f)[axis] for f in range(c.NF)]), axis


def diagonal_fold(c, phi):
    """1 x 1 only: vertex b = (0, 1) turned by phi about the diagonal a - c"""
    assert c.N == 1 and c.M == 1
    x, _, _ = flat(c)
    ax = (x[3] - x[0]) / np.linalg.norm(x[3] - x[0])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) - np.sin(phi) * K + (1 - np.cos(phi)) * K @ K   # (turned by -phi: the sense that the reference's convention calls +phi)
    x[1] = x[0] + R @ (x[1] - x[0])
    return x, np.array([0, 1]), None


def bump(c, amp=0.3, seed=0):
    i, j = grid(c)
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 4)
    x, _, _ = flat(c)
    x[:, 2] = amp * c.dx * (np.sin(1.3 * i + ph[0]) * np.cos(0.9 * j + ph[1]) + 0.5 * np.sin(2.1 * j + 0.7 * i + ph[2]))
    x[:, :2] += 0.05 * c.dx * rng.normal(size=(len(i), 2))
    return x, np.full(c.NF, -1), None


def fold_ref(c, phi, axis=0, line=1):
    """reference angles equal to phi on the hinges of the fold line (both wings' slots), zero elsewhere"""
    ra = np.zeros((c.NF, 3))
    for f, l in c.hinges:
        v, i2, _, _, _ = c.hinge_verts(f, l)
        if _cell_of_face(c, f)[axis] != _cell_of_face(c, i2)[axis]:
            s = [(w // (c.M + 1), w % (c.M + 1))[axis] for w in v[1:3]]
            if s[0] == line and s[1] == line:
                ra[f, l] = phi
    return ra


def random_ref(c, seed, amp=0.3):
    return np.random.default_rng(seed).uniform(-amp, amp, (c.NF, 3))


def make_state(name, parts):
    """parts: list of (ClothTables, (x, pieces, ruling), ra, rotation or None, translation)"""
    xs, ras, pcs, rul, cl = [], [], [], [], []
    for c, (x, pieces, ruling), ra, R, t in parts:
        assert c.v_offset == sum(len(v) for v in xs)
        x = x if R is None else x @ np.asarray(R).T
        xs.append(x + np.asarray(t, float)); ras.append(np.asarray(ra, float)); pcs.append(pieces); rul.append(ruling); cl.append(c)
    return State(name, cl, np.concatenate(xs), ras, pcs, rul)


# ------------------------------------------------------------------------------------------------ decisions
def _by_construction(st, i, kind, f, l, nb):
    """the sign quantity n2 . e is zero in exact arithmetic for the state as built: both end points of e are vertices of the neighbour, or own face
    and neighbour lie in one exactly planar piece (an exactly flat sheet is one piece), or the state is a cylinder and e runs along its ruling"""
    c = st.cloths[i]
    ends = (c.f2v[f, (l + 1) % 2], c.f2v[f, l])
    if all(v in c.f2v[nb] for v in ends):
        return True
    if st.pieces[i][f] >= 0 and st.pieces[i][f] == st.pieces[i][nb]:
        return True
    ax = st.ruling[i]
    if ax is not None:
        s = [(v // (c.M + 1), v % (c.M + 1))[ax] for v in ends]
        return s[0] == s[1]
    return False


def decisions(st, xp):
    out = []
    for i, c in enumerate(st.cloths):
        dec = []
        with mp.workdps(50):
            evaluate(xp, c, st.local(i), st.ra[i], dec=dec)
        out.append(dec)
    return out


def decisions_safe(st):
    """every decision of the state is zero by construction (sign test only, and then below 1e-12, four decades inside the engine's 1e-10) or
    at least 1e-6 from its threshold, on the same side in both backends.  A condition on the inputs of a GPU test, not a tolerance."""
    dm, df = decisions(st, MP), decisions(st, F64)
    for i in range(len(st.cloths)):
        assert len(dm[i]) == len(df[i])
        for a, b in zip(dm[i], df[i]):
            assert a[:-1] == b[:-1]
            da, db = float(a[-1]), float(b[-1])
            if a[0] == "sign" and _by_construction(st, i, *a[:4]):
                assert abs(da - SIGN_TOL) <= 1e-12 and abs(db - SIGN_TOL) <= 1e-12, (st.name, i, a, b)
            else:
                assert abs(da) >= SAFE and abs(db) >= SAFE and (da > 0) == (db > 0), (st.name, i, a, b)
    return True


# ------------------------------------------------------------------------------------------------ float64 errors
def rotations():
    """the six coordinate permutations as proper rotations (an odd one negates its first row: a mirror image would flip every dihedral): signed
    permutation matrices, exact in floating point"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        R = np.zeros((3, 3))
        for r in range(3):
            R[r, p[r]] = 1.0
        if np.linalg.det(R) < 0:
            R[0] = -R[0]
        out.append(R)
    return out


def jitters(x, n=8, seed=0):
    """n copies of x with every coordinate moved by one ulp, up or down"""
    rng = np.random.default_rng(seed)
    return [np.nextafter(x, np.where(rng.integers(0, 2, x.shape) == 1, np.inf, -np.inf)) for _ in range(n)]


def _back(ev, R):
    """quantities computed at x R^T, turned back: vectors v R, blocks R^T B R"""
    out = dict(ev)
    for q in ("gS", "gA", "gS1", "gA1", "gB", "gB1", "g"):
        out[q] = ev[q] @ R
    out["K3"] = np.einsum("ja,fsjk,kb->fsab", R, ev["K3"], R)
    for q in ("HS", "HA", "HB", "G"):
        out[q] = np.einsum("ja,fljmk,kb->flamb", R, ev[q], R)
    return out


def split(a):
    """mp array -> (hi, lo) float arrays with hi + lo = a to 1e-32"""
    a = np.asarray(a, dtype=object)
    hi = np.array([float(v) for v in a.ravel()]).reshape(a.shape)
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(a.ravel(), hi.ravel())]).reshape(a.shape)
    return hi, lo


def diff(got, hl):
    """got - (hi + lo) in float64, exact to the second order"""
    return (np.asarray(got, float) - hl[0]) - hl[1]


class Reference:
    """mp values of every element of a state and the float64 evaluations that e64 is taken from (all against the mp values of the state itself):
    the state and its coordinate rotations, eight copies with every coordinate moved by one ulp, and the state with the cosine n1 . n2 of every
    face pair that is coplanar by construction (equal `pieces` label) moved by +1 and by -1 ulp.  The last two are there because such a pair keeps
    c = 1 - (0 .. 2) ulp whatever the last bits of the input, an ulp of c is 1e-8 rad through the series branch, and moving the coordinates does not
    reach that rounding.  Every other pair is evaluated as it stands."""
    def __init__(self, st):
        self.st = st
        with mp.workdps(50):
            self.mp = [evaluate(MP, c, st.local(i), st.ra[i]) for i, c in enumerate(st.cloths)]
            self.hl = [{q: split(v) for q, v in ev.items()} for ev in self.mp]
        self.f64 = []
        with np.errstate(all="ignore"):
            for i, c in enumerate(st.cloths):
                vs = [_back(evaluate(F64, c, st.local(i) @ R.T, st.ra[i]), R) for R in rotations()]
                vs += [evaluate(F64, c, st.local(i, xj), st.ra[i]) for xj in jitters(st.x, seed=len(st.x))]
                flat_pairs = {(f, int(c.cf[f, l])) for f in range(c.NF) for l in range(3)
                              if c.cf[f, l] != -1 and st.pieces[i][f] >= 0 and st.pieces[i][f] == st.pieces[i][c.cf[f, l]]}
                vs += [evaluate(F64, c, st.local(i), st.ra[i], cos_ulps=(k, flat_pairs)) for k in (1, -1)]
                self.f64.append(vs)

    def e64(self, i, fun, axes):
        """largest Frobenius norm (over `axes`) of fun(f64 evaluation) - fun(mp) over the evaluations; fun maps an evaluation dict (float arrays, or
        (hi, lo) pairs via `parts`) to an array"""
        want = fun(self.hl[i], 0), fun(self.hl[i], 1)
        worst = None
        for ev in self.f64[i]:
            d = (fun(ev, None) - want[0]) - want[1]
            n = np.sqrt((d * d).sum(axis=axes)) if axes else np.abs(d)
            worst = n if worst is None else np.fmax(worst, n)   # (fmax: a NaN evaluation does not erase the others)
        return worst


@functools.lru_cache(maxsize=None)
def reference(key):
    return Reference(STATES[key]())


STATES = {}   # {key: function returning a State}: filled by _register() below


# ------------------------------------------------------------------------------------------------ the engine context
def cloth_context(cloths, nv, frozen=None):
    """engine context of cloths only: no faces table, no pairs, gravity 0, mass 1e-30 (m / dt^2 is lost in every block), tables from init_mesh"""
    from thinshelllab_amd.context import TslContext
    return TslContext(tot_NV=nv, dt=DT, mass=np.full(nv, MASS), gravity=np.zeros((nv, 3)),
                      frozen=np.zeros(3 * nv, np.int32) if frozen is None else frozen, cloths=[c.desc for c in cloths])


# ------------------------------------------------------------------------------------------------ what an assembly must give
COMBOS = {"Kl": (1, 0, 0), "Ka": (0, 1, 0), "Kb": (0, 0, 1), "all": (1, 1, 1)}


def _sel(ev, part, names):
    """sum of the named arrays of an evaluation (float arrays; part 0 / 1: the hi / lo halves of the mp values)"""
    out = None
    for q in names:
        a = ev[q] if part is None else ev[q][part]
        out = a if out is None else out + a
    return out


def _names(combo, S, A, B):
    return [q for q, on in zip((S, A, B), combo) if on and q is not None]


def _fn(a):
    return np.sqrt((np.asarray(a, float) ** 2).sum())


class Expected:
    """what expected() returns: mp values and bounds of everything the engine returns for a state with the constants switched by `combo` (Kl, Ka, Kb
    on / off), the projection `spd` and the frozen vertices.  A: (hi, lo) of the dense matrix, Ab: bound per vertex pair, pattern: vertex pairs
    that some element couples; g: (hi, lo) of the gradient, gb: bound per vertex; E, Eb: energy and its bound; keys: {key: (mp sum, bound)} for
    the vector p; free: mask of the free vertices; nv"""
    __slots__ = ("A", "Ab", "pattern", "g", "gb", "E", "Eb", "keys", "p", "free", "nv")


@functools.lru_cache(maxsize=None)
def _clamped_springs(ref):
    """per cloth: mp HS with every spring block eigen-clamped, (nf, 3) |K3|_F"""
    out = []
    with mp.workdps(50):
        for i, c in enumerate(ref.st.cloths):
            K3 = ref.mp[i]["K3"]
            HS = np.array([scatter_springs(MP, [clamp3(MP, K3[f][s].tolist()) for s in range(3)]) for f in range(c.NF)], dtype=object)
            out.append((HS.reshape(c.NF, 3, 3, 3, 3), np.sqrt((ref.hl[i]["K3"][0] ** 2).sum(axis=(2, 3)))))
    return out


def _bnd(e64, norm, extra=0.0):
    """tet_numpy.bound on arrays"""
    return 8 * np.maximum(e64 + extra, 4 * U * norm)


@functools.lru_cache(maxsize=None)
def _face_blocks(ref, combo_name, spd):
    """per cloth (mp face blocks [f, l, j, m, k] as the engine forms them under `spd`, bound per sub-block [f, l, m]), or None without faces' terms"""
    from tet_numpy import project9
    combo = COMBOS[combo_name]
    names = _names(combo, "HS", "HA", "HB")
    out = []
    with mp.workdps(50):
        for i, c in enumerate(ref.st.cloths):
            if not names:
                out.append(None)
                continue
            evm = ref.mp[i]
            e_sub = ref.e64(i, lambda ev, part: _sel(ev, part, names), (2, 4))
            T = _sel(evm, None, names)
            extra = np.zeros((c.NF, 3, 3)); e_add = np.zeros((c.NF, 3, 3))
            if spd and combo[0]:
                HSc, nK = _clamped_springs(ref)[i]
                eK = ref.e64(i, lambda ev, part: _sel(ev, part, ["K3"]), (2, 3))
                T = T - evm["HS"] + HSc
                for s in range(3):
                    for l in (s, (s + 1) % 3):
                        for m in (s, (s + 1) % 3):
                            extra[:, l, m] += 64 * U * nK[:, s]; e_add[:, l, m] += eK[:, s]
            if spd == 2:   # the projection is non-expansive on the whole block only: every sub-block takes the whole block's error
                e_all = ref.e64(i, lambda ev, part: _sel(ev, part, names), (1, 2, 3, 4))
                n9 = np.array([float(fro(T[f])) for f in range(c.NF)])
                T = np.array([project9(MP, T[f].reshape(9, 9).tolist()) for f in range(c.NF)], dtype=object).reshape(c.NF, 3, 3, 3, 3)
                extra = np.repeat((extra.sum(axis=(1, 2)) / 4 + 64 * U * n9)[:, None], 9, 1).reshape(c.NF, 3, 3)
                e_add = np.repeat((e_add.sum(axis=(1, 2)) / 4)[:, None], 9, 1).reshape(c.NF, 3, 3)
                e_sub = np.repeat(e_all[:, None], 9, 1).reshape(c.NF, 3, 3)
            nrm = np.sqrt((split(T)[0] ** 2).sum(axis=(2, 4)))
            out.append((T, _bnd(e_sub + e_add, nrm, extra)))
    return out


@functools.lru_cache(maxsize=None)
def expected(ref, combo_name, spd, frozen_verts=(), p_seed=None):
    st, combo = ref.st, COMBOS[combo_name]
    sl, sa, sb = combo
    nv = st.nv
    out = Expected()
    fb = _face_blocks(ref, combo_name, spd)
    with mp.workdps(50):
        zero = mp.mpf(0)
        blocks, bb = {}, {}
        grad = np.full((nv, 3), zero, dtype=object); gb = np.zeros(nv)
        E, Eb = zero, 0.0
        p = None if p_seed is None else np.random.default_rng(p_seed).normal(size=(nv, 3))
        free = np.ones(nv, bool); free[list(frozen_verts)] = False
        keys = {}
        for i, c in enumerate(st.cloths):
            evm, hl, off = ref.mp[i], ref.hl[i], c.v_offset
            gv = c.f2v + off
            # ---- faces: block
            if fb[i] is not None:
                T, bnd = fb[i]
                for f in range(c.NF):
                    for l in range(3):
                        for m in range(3):
                            k = (gv[f, l], gv[f, m])
                            blocks[k] = blocks.get(k, 0) + T[f, l, :, m, :]
                            bb[k] = bb.get(k, 0.0) + bnd[f, l, m]
            # ---- faces: gradient, energy, keys
            names = _names(combo, "gS", "gA", None)
            if names:
                G = _sel(evm, None, names)
                bnd = _bnd(ref.e64(i, lambda ev, part: _sel(ev, part, names), (2,)), np.sqrt((_sel(hl, 0, names) ** 2).sum(axis=2)))
                for f in range(c.NF):
                    for l in range(3):
                        grad[gv[f, l]] += G[f, l]; gb[gv[f, l]] += bnd[f, l]
                en = _names(combo, "eS", "eA", None)
                E += sum(_sel(evm, None, en)); Eb += ref.e64(i, lambda ev, part: _sel(ev, part, en), None).sum()
            # ---- hinges
            hv = np.array([c.hinge_verts(f, l)[0] for f, l in c.hinges], int).reshape(-1, 4) + off
            if sb and len(hv):
                bnd = _bnd(ref.e64(i, lambda ev, part: _sel(ev, part, ["G"]), (2, 4)), np.sqrt((hl["G"][0] ** 2).sum(axis=(2, 4))))
                bg = _bnd(ref.e64(i, lambda ev, part: _sel(ev, part, ["gB"]), (2,)), np.sqrt((hl["gB"][0] ** 2).sum(axis=2)))
                for h in range(len(hv)):
                    for a in range(4):
                        grad[hv[h, a]] += evm["gB"][h, a]; gb[hv[h, a]] += bg[h, a]
                        for b in range(4):
                            k = (hv[h, a], hv[h, b])
                            blocks[k] = blocks.get(k, 0) + evm["G"][h, a, :, b, :]
                            bb[k] = bb.get(k, 0.0) + bnd[h, a, b]
                E += sum(evm["eB"]); Eb += ref.e64(i, lambda ev, part: _sel(ev, part, ["eB"]), None).sum()
            # ---- per-key sums: -sum over the free dofs of p . d(gradient)/d(key)
            if p is not None:
                for key, q, verts in (("Kl", "gS1", gv), ("Ka", "gA1", gv), ("Kb", "gB1", hv)):
                    pe = p[verts] * free[verts][..., None]
                    w = -sum((np.array([[mp.mpf(float(v)) for v in r] for r in pe.reshape(-1, 3)], dtype=object).reshape(pe.shape) * evm[q]).ravel()) if len(verts) else zero
                    e = (np.sqrt((pe ** 2).sum(axis=(1, 2))) * ref.e64(i, lambda ev, part: _sel(ev, part, [q]), (1, 2))).sum() if len(verts) else 0.0
                    keys["cloth%d.%s" % (i, key)] = (w, bound(mp.mpf(e), abs(w)))
        # ---- frozen rule and mass term, dense (hi, lo) and bounds
        m = mp.mpf(MASS) / mp.mpf(DT) ** 2
        Wh, Wl = np.zeros((nv, 3, nv, 3)), np.zeros((nv, 3, nv, 3))
        Wb = np.zeros((nv, nv)); pat = np.zeros((nv, nv), bool)
        md = np.diag([m, m, m]) + np.full((3, 3), zero, dtype=object)
        for v in range(nv):
            if (v, v) not in blocks:
                blocks[(v, v)] = 0 * md; bb[(v, v)] = 0.0
        for (a, b), blk in blocks.items():
            pat[a, b] = True
            if free[a] and free[b]:
                Wh[a, :, b, :], Wl[a, :, b, :] = split(blk + md if a == b else blk)
                Wb[a, b] = bb[(a, b)]
            elif a == b:
                Wh[a, :, b, :], Wl[a, :, b, :] = split(md)
            if a == b:
                Wb[a, a] = max(Wb[a, a], float(bound(0, m * mp.sqrt(3))))
        grad[~free] = zero; gb[~free] = 0.0
        out.A, out.Ab, out.pattern = (Wh.reshape(3 * nv, 3 * nv), Wl.reshape(3 * nv, 3 * nv)), Wb, pat
        out.g, out.gb = split(grad), gb
        out.E, out.Eb = E, float(bound(mp.mpf(Eb), abs(E)))
        out.keys, out.p, out.free, out.nv = keys, p, free, nv
    return out


def check_assembly(exp, A, g, R, tag, psd=False):
    """every vertex-pair block of the dense matrix A and every vertex of the gradient g against mp: largest error / bound into the Ratios R;
    entries outside the cloths' pattern must be zero; psd: the matrix is a sum of projected blocks and so PSD to within the summed bounds"""
    nv = exp.nv
    d = diff(A, exp.A).reshape(nv, 3, nv, 3)
    err = np.sqrt((d * d).sum(axis=(1, 3)))
    A4 = np.asarray(A).reshape(nv, 3, nv, 3)
    assert not A4.transpose(0, 2, 1, 3)[~exp.pattern].any(), tag
    on = exp.Ab > 0
    assert not err[~on].any(), (tag, "frozen or empty blocks must be exact")
    R.add("block " + tag, float((err[on] / exp.Ab[on]).max()), 1.0)
    if g is not None:
        eg = np.sqrt((diff(np.asarray(g).reshape(nv, 3), exp.g) ** 2).sum(axis=1))
        on = exp.gb > 0
        assert not eg[~on].any(), tag
        if on.any():
            R.add("gradient", float((eg[on] / exp.gb[on]).max()), 1.0)
    if psd:
        S = 0.5 * (np.asarray(A) + np.asarray(A).T)
        assert np.linalg.eigvalsh(S).min() >= -exp.Ab.sum(), tag


def f64_assembly(ref, combo_name, k=1):
    """the harness's own input: the k-th float64 evaluation (another rotation: other rounding) assembled in float64, unprojected, no frozen vertices"""
    st, combo = ref.st, COMBOS[combo_name]
    nv = st.nv
    A = np.zeros((nv, 3, nv, 3)); g = np.zeros((nv, 3)); E = 0.0
    for i, c in enumerate(st.cloths):
        ev, gv = ref.f64[i][k], c.f2v + c.v_offset
        names, gn, en = _names(combo, "HS", "HA", "HB"), _names(combo, "gS", "gA", None), _names(combo, "eS", "eA", None)
        for f in range(c.NF):
            for l in range(3):
                if gn:
                    g[gv[f, l]] += _sel(ev, None, gn)[f, l]
                for m in range(3):
                    if names:
                        A[gv[f, l], :, gv[f, m], :] += _sel(ev, None, names)[f, l, :, m, :]
        if en:
            E += _sel(ev, None, en).sum()
        if combo[2]:
            for h, (f, l) in enumerate(c.hinges):
                hv = np.array(c.hinge_verts(f, l)[0]) + c.v_offset
                for a in range(4):
                    g[hv[a]] += ev["gB"][h, a]
                    for b in range(4):
                        A[hv[a], :, hv[b], :] += ev["G"][h, a, :, b, :]
            E += ev["eB"].sum()
    A = A.reshape(3 * nv, 3 * nv)
    A[np.arange(3 * nv), np.arange(3 * nv)] += MDT2
    return A, g, E


# ------------------------------------------------------------------------------------------------ the meshes and states of the GPU tests
DXS = {"dx150": 1.0 / 150, "dx1e-4": 1e-4}
PI_NEAR = np.pi - 1e-3
FOLDS = {"90": np.pi / 2, "170": np.radians(170.0), "pi": PI_NEAR}
SECOND = dict(Kl=700.0, Ka=1300.0, Kb=60.0)   # the constants of every second cloth


def _fold_axis(N, M):
    return (0, 1) if N >= 2 else (1, 1)


def _first(N, M, dx, kind, arg=None, ref="0"):
    """(tables, geometry, reference angles, rotation) of the first cloth of a state"""
    c = ClothTables(N, M, dx)
    R, ra = None, np.zeros((c.NF, 3))
    if kind in ("rest", "rest_rot"):
        geo, R = flat(c), (R1 if kind == "rest_rot" else None)
    elif kind == "ripple":
        geo = ripple(c, arg, 0 if N >= 2 else 1)
    elif kind == "fold":
        if N == 1 and M == 1:
            geo = diagonal_fold(c, arg)
            ra[0, 1] = {"0": 0.0, "same": arg, "opp": -arg}[ref]
        else:
            ax, line = _fold_axis(N, M) if max(N, M) < 8 else (0, N // 2)
            geo = fold(c, arg, ax, line)
            ra = fold_ref(c, {"0": 0.0, "same": arg, "opp": -arg}[ref], ax, line)
    elif kind == "stretch":
        geo, R = flat(c, 1.5, 1.5), R1
    elif kind == "compress":
        geo = flat(c, 0.5, 0.5)
    elif kind == "sliver":
        geo = flat(c, shear=np.sqrt(999.0) - 1.0)   # the sheared diagonal (1 + t, 1) dx has length dx sqrt(1000) and altitude dx / sqrt(1000): 1e-3 of its length
    elif kind == "bump":
        geo = bump(c, 0.3, seed=N * 10 + M)
    return c, geo, ra, R


def _second(N, M, dx, off):
    c = ClothTables(N, M, 0.8 * dx, v_offset=off, k_angle=2.5, **SECOND)
    geo = diagonal_fold(c, 0.7) if (N, M) == (1, 1) else fold(c, -1.2, 1, 1)
    return c, geo, random_ref(c, seed=N + M), R2


def _state(name, N, M, dx, kind, arg=None, ref="0", second=None):
    c, geo, ra, R = _first(N, M, dx, kind, arg, ref)
    parts = [(c, geo, ra, R, (0.0, 0.0, 0.0))]
    if second:
        c2, geo2, ra2, R2_ = _second(second[0], second[1], dx, c.NV)
        parts.append((c2, geo2, ra2, R2_, (0.0, 0.0, 20 * dx)))
    return make_state(name, parts)


def _register():
    full = [("rest", "rest", None, "0"), ("rest_rot", "rest_rot", None, "0"), ("ripple1.0e-4", "ripple", 1.0e-4, "0"),
            ("ripple1.3e-3", "ripple", 1.3e-3, "0"), ("ripple1.5e-3", "ripple", 1.5e-3, "0"), ("stretch", "stretch", None, "0"),
            ("compress", "compress", None, "0"), ("sliver", "sliver", None, "0"), ("bump", "bump", None, "0")]
    for fn, ang in FOLDS.items():
        for sg in (1, -1):
            for ref in ("0", "same", "opp"):
                full.append(("fold%s%s_ref%s" % ("+" if sg > 0 else "-", fn, ref), "fold", sg * ang, ref))
    no_ripple = [t for t in full if t[1] != "ripple"]     # 1 x 1 has one strip: a zigzag needs a grid line between two
    large = [("ripple1.5e-3", "ripple", 1.5e-3, "0"), ("fold+90_ref0", "fold", np.pi / 2, "0")]
    middle = large + [("bump", "bump", None, "0"), ("compress", "compress", None, "0"), ("fold-pi_refopp", "fold", -PI_NEAR, "opp")]
    table = [((3, 2), None, full), ((1, 1), None, no_ripple), ((2, 1), None, full), ((1, 2), None, full),
             ((8, 8), None, middle), ((8, 8), (1, 1), middle), ((10, 10), None, large), ((10, 10), (3, 2), large)]
    for (N, M), second, states in table:
        mesh = "%dx%d" % (N, M) + ("+%dx%d" % second if second else "")
        for dn, dx in DXS.items():
            for sn, kind, arg, ref in states:
                key = "%s/%s/%s" % (mesh, dn, sn)
                STATES[key] = functools.partial(_state, key, N, M, dx, kind, arg, ref, second)
    # update_ref_angle: folds at 0.5, 0.99, 1.01 and 2 times the plastic threshold (0.5 rad), both signs
    for fac in (0.5, 0.99, 1.01, 2.0):
        for sg in (1, -1):
            key = "plastic/%s%g" % ("+" if sg > 0 else "-", fac)
            STATES[key] = functools.partial(_plastic_state, key, sg * fac)


PLASTIC = 0.5


def _plastic_state(name, fac):
    c = ClothTables(3, 2, DXS["dx150"], k_angle=PLASTIC)
    c2 = ClothTables(2, 1, 0.8 * DXS["dx150"], v_offset=c.NV, k_angle=0.8 * PLASTIC, **SECOND)
    return make_state(name, [(c, fold(c, fac * PLASTIC, 0, 1), np.zeros((c.NF, 3)), None, (0.0, 0.0, 0.0)),
                             (c2, fold(c2, -fac * 0.8 * PLASTIC, 0, 1), np.zeros((c2.NF, 3)), R2, (0.0, 0.0, 0.1))])


_register()
GPU_KEYS = [k for k in STATES if not k.startswith("plastic/")]
PLASTIC_KEYS = [k for k in STATES if k.startswith("plastic/")]


def frozen_of(st):
    """the three frozen vertices of the frozen runs"""
    return (0, st.nv // 2, st.nv - 1)
