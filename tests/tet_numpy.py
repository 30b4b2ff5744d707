"""Restatement of one tetrahedron of the two FEM materials (csrc/k_fem.hpp, k_pg_tet of csrc/k_param.hpp) for tests/test_tet_numpy.py and
tests/test_gpu_tet_elements.py, written from the reference's formulas (engine/model_elastic_tactile.py = kind 0, engine/model_elastic_offset.py
= kind 1), not from the kernels.  Every function takes a backend `xp`: MP (mpmath at 50 digits, the reference proper) or F64 (NumPy float64
scalars, the same formulas in the same plain order: it only measures what double precision delivers, see bound()).  The 3 x 3 algebra is
spelled out on lists of scalars so that both backends run the very same sequence of operations.  Nothing here calls the GPU except
tet_context(), which builds an engine context from tables (elastic bodies only, as ee_numpy.bar_context).

Conventions restated:
- F = Ds B, Ds = columns x_i - x_3 (i = 0..2), B = (rest Ds)^-1 as the 9 doubles the engine is given (row major), W = rest volume;
- gradient of vertex i, component j = W (P B^T)[j][i]; vertex 3 takes minus the sum; force = -gradient;
- kind 0 (tactile): Psi = mu/2 (I1 - 3) + lam/2 (J - alpha)^2; the reference writes P and dP with F^-1 ("literal"), which equals the
  polynomial P = mu F + lam (J - alpha) cof F, dP = mu dF + lam dJ cof F + lam (J - alpha) d(cof F) wherever F^-1 exists; the polynomial
  is the reference at J = 0 and next to it.  Block entry [(n, dim)][(i, j)] = d grad(i, j) / d x(n, dim): row = variable;
- kind 1 (box), literal: F^-1 from the raw F, log(max(J, 0.01)) in gradient and block, log(max(0.01, J)) in the energy, and the term
  lam tr(F^-1 dF) F^-T kept below the clamp (where the block is no longer the derivative of the gradient).  The reference scatters
  row = (vertex j, comp r), column = (n, dim);
- vertex 3: minus the row and column sums of the 9 x 9 block;
- SPD projection (symmetrise, eigen-decompose, clamp at 0, rebuild) of the 9 x 9 block: spd 1 on kind 0, spd 2 on both kinds;
- frozen rule (the `masked` convention of tsl_contact_blocks_export, k_mask_matrix): rows and columns of frozen dofs are removed, the
  diagonal entry of a frozen dof is m / dt^2; frozen entries of the assembled gradient are zero."""
import functools
import itertools

import mpmath as mp
import numpy as np

U = 2.0 ** -53
J_CLAMP = "0.01"


class MP:
    """mpmath, 50 digits"""
    name = "mp"

    @staticmethod
    def num(v):
        return mp.mpf(v) if isinstance(v, str) else mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v

    log = staticmethod(mp.log)
    sqrt = staticmethod(mp.sqrt)
    acos = staticmethod(mp.acos)

    @staticmethod
    def eigh(A):
        w, V = mp.eigsy(mp.matrix(A))
        n = len(A)
        return [w[i] for i in range(n)], [[V[i, j] for j in range(n)] for i in range(n)]


class F64:
    """IEEE double scalars"""
    name = "f64"

    @staticmethod
    def num(v):
        return np.float64(v)

    log = staticmethod(np.log)
    sqrt = staticmethod(np.sqrt)
    acos = staticmethod(np.arccos)

    @staticmethod
    def eigh(A):
        w, V = np.linalg.eigh(np.array(A, dtype=np.float64))
        return list(w), [list(r) for r in V]


def with_mp(fun):
    """run with 50 digits and leave the caller's precision as it was"""
    @functools.wraps(fun)
    def g(*a, **k):
        with mp.workdps(50):
            return fun(*a, **k)
    return g


# ------------------------------------------------------------------------------------------------ 3 x 3 algebra on lists
def _zeros(xp, n, m):
    return [[xp.num(0) for _ in range(m)] for _ in range(n)]


def _mat(xp, a):
    a = np.asarray(a, dtype=object) if not isinstance(a, list) else a
    return [[xp.num(a[i][j]) for j in range(len(a[0]))] for i in range(len(a))]


def _mul(a, b):
    n, m, k = len(a), len(b[0]), len(b)
    out = []
    for i in range(n):
        row = []
        for j in range(m):
            s = a[i][0] * b[0][j]
            for q in range(1, k):
                s = s + a[i][q] * b[q][j]
            row.append(s)
        out.append(row)
    return out


def _T(a):
    return [[a[j][i] for j in range(len(a))] for i in range(len(a[0]))]


def _cof(a, b=None):
    """cofactor matrix of a (b None), or the bilinear form whose diagonal it is: cof(a)[i][j] = a[i+1][j+1] a[i+2][j+2] - a[i+1][j+2] a[i+2][j+1]
    with cyclic indices; _cof(a, b) takes the first factor of each product from a and the second from b"""
    b = a if b is None else b
    return [[a[(i + 1) % 3][(j + 1) % 3] * b[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * b[(i + 2) % 3][(j + 1) % 3]
             for j in range(3)] for i in range(3)]


def _det(a):
    c = _cof(a)
    return a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2]


def _inv(a):
    """adjugate over determinant (what a closed-form 3 x 3 inverse is)"""
    c, d = _cof(a), _det(a)
    return [[c[j][i] / d for j in range(3)] for i in range(3)]


def _ddot(a, b):
    s = a[0][0] * b[0][0]
    for i in range(3):
        for j in range(3):
            if i or j:
                s = s + a[i][j] * b[i][j]
    return s


def _trace(a):
    return a[0][0] + a[1][1] + a[2][2]


def _lin(xp, terms):
    """sum of coefficient * matrix"""
    out = _zeros(xp, 3, 3)
    for i in range(3):
        for j in range(3):
            s = terms[0][0] * terms[0][1][i][j]
            for c, m in terms[1:]:
                s = s + c * m[i][j]
            out[i][j] = s
    return out


# ------------------------------------------------------------------------------------------------ one element
class Material:
    def __init__(self, kind, mu, lam, alpha=None):
        self.kind, self.mu, self.lam = int(kind), float(mu), float(lam)
        self.alpha = float(1.0 + mu / lam if alpha is None else alpha) if kind == 0 else 0.0   # Elastic.__init__: alpha = 1 + mu / lam (tactile)

    def consts(self, xp):
        return xp.num(self.mu), xp.num(self.lam), xp.num(self.alpha)


def deformation(xp, x, B):
    """F = Ds B and B as scalar lists; x: (4, 3), B: 9 numbers row major"""
    x = _mat(xp, np.asarray(x, dtype=object).reshape(4, 3).tolist())
    Bm = _mat(xp, np.asarray(B, dtype=object).reshape(3, 3).tolist())
    Ds = [[x[c][r] - x[3][r] for c in range(3)] for r in range(3)]
    return _mul(Ds, Bm), Bm


def energy(xp, x, B, W, mat):
    F, _ = deformation(xp, x, B)
    mu, lam, alpha = mat.consts(xp)
    I1 = _trace(_mul(_T(F), F))
    J = _det(F)
    if mat.kind == 0:
        phi = mu / 2 * (I1 - 3) + lam / 2 * (J - alpha) ** 2
    else:
        c = xp.num(J_CLAMP)
        lj = xp.log(c if c > J else J)   # log(max(0.01, J))
        phi = mu / 2 * (I1 - 3) - mu * lj + lam / 2 * lj * lj
    return xp.num(W) * phi


def _clampJ(xp, J):
    c = xp.num(J_CLAMP)
    return J if J > c else c   # max(J, 0.01)


def pk1(xp, F, mat, form="poly", part=None):
    """first Piola-Kirchhoff stress; part "mu" / "lam": its derivative by that parameter with alpha held fixed"""
    mu, lam, alpha = mat.consts(xp)
    one, zero = xp.num(1), xp.num(0)
    cm, cl = (mu, lam) if part is None else ((one, zero) if part == "mu" else (zero, one))
    J = _det(F)
    if mat.kind == 0:
        if form == "poly":
            return _lin(xp, [(cm, F), (cl * (J - alpha), _cof(F))])
        FiT = _T(_inv(F))   # model_elastic_tactile.py:146-149
        return _lin(xp, [(cm, F), (cl * (J - alpha) * J, FiT)])
    FiT = _T(_inv(F))       # model_elastic_offset.py:190-193
    lj = xp.log(_clampJ(xp, J))
    return _lin(xp, [(cm, F), (-cm, FiT), (cl * lj, FiT)])


def _vertex_vector(xp, P, Bm, W):
    """12 numbers from W P B^T: vertex i, comp j = [j][i]; vertex 3 = minus the sum"""
    H = _mul(P, _T(Bm))
    W = xp.num(W)
    g = [[W * H[j][i] for j in range(3)] for i in range(3)]
    g.append([-(g[0][j] + g[1][j] + g[2][j]) for j in range(3)])
    return [g[i][j] for i in range(4) for j in range(3)]


def gradient(xp, x, B, W, mat, form="poly"):
    F, Bm = deformation(xp, x, B)
    return _vertex_vector(xp, pk1(xp, F, mat, form), Bm, W)


def dgrad_dparam(xp, x, B, W, mat, part):
    """d(gradient)/d(mu) or /d(lam), alpha fixed; d(force)/d(key) of tsl_param_grad_keys is minus this"""
    F, Bm = deformation(xp, x, B)
    return _vertex_vector(xp, pk1(xp, F, mat, "poly", part), Bm, W)


def dpk1(xp, F, mat, dF, form="poly", drop_trace_term=False):
    mu, lam, alpha = mat.consts(xp)
    J = _det(F)
    if mat.kind == 0:
        if form == "poly":
            C = _cof(F)
            dJ = _ddot(C, dF)
            dC = _lin(xp, [(xp.num(1), _cof(F, dF)), (xp.num(1), _cof(dF, F))])
            return _lin(xp, [(mu, dF), (lam * dJ, C), (lam * (J - alpha), dC)])
        Fi = _inv(F); FiT = _T(Fi)   # model_elastic_tactile.py:101-107, signs folded (the reference forms -dP)
        dTr = _trace(_mul(Fi, dF))
        X = _mul(_mul(FiT, _T(dF)), FiT)
        return _lin(xp, [(mu, dF), (lam * 2 * J ** 2 * dTr, FiT), (-lam * alpha * J * dTr, FiT), (-lam * (J - alpha) * J, X)])
    Fi = _inv(F); FiT = _T(Fi)       # model_elastic_offset.py:120-145
    lj = xp.log(_clampJ(xp, J))
    dTr = _trace(_mul(Fi, dF))
    X = _mul(_mul(FiT, _T(dF)), FiT)
    terms = [(mu, dF), (mu - lam * lj, X)]
    if not drop_trace_term:
        terms.append((lam * dTr, FiT))
    return _lin(xp, terms)


def block9(xp, x, B, W, mat, form="poly", drop_trace_term=False):
    """the 9 x 9 block over vertices 0..2 in matrix convention K[row dof][column dof] as the reference scatters it"""
    F, Bm = deformation(xp, x, B)
    BT = _T(Bm)
    Wn = xp.num(W)
    K = _zeros(xp, 9, 9)
    for n in range(3):
        for dim in range(3):
            dD = _zeros(xp, 3, 3)
            dD[dim][n] = xp.num(1)
            dF = _mul(dD, Bm)
            dH = _mul(dpk1(xp, F, mat, dF, form, drop_trace_term), BT)
            for i in range(3):
                for j in range(3):
                    v = Wn * dH[j][i]
                    if mat.kind == 0:
                        K[n * 3 + dim][i * 3 + j] = v     # H_e[n * 3 + dim, i * 3 + j], scattered row = first index
                    else:
                        K[i * 3 + j][n * 3 + dim] = v     # add_H(idx_j * 3 + r, ind(n, dim), ...)
    return K


def project9(xp, K):
    """symmetrise, eigen-decompose, clamp at 0, rebuild"""
    S = [[(K[i][j] + K[j][i]) / 2 for j in range(9)] for i in range(9)]
    w, V = xp.eigh(S)
    zero = xp.num(0)
    out = _zeros(xp, 9, 9)
    for i in range(9):
        for j in range(9):
            s = zero
            for e in range(9):
                if w[e] > zero:
                    s = s + w[e] * V[i][e] * V[j][e]
            out[i][j] = s
    return out


def clamps(mat, spd):
    return (mat.kind == 0 and spd >= 1) or spd == 2


def block12(xp, K9):
    """vertex 3 = minus the row and column sums"""
    K = _zeros(xp, 12, 12)
    for r in range(9):
        for c in range(9):
            K[r][c] = K9[r][c]
    for r in range(9):
        for j in range(3):
            K[r][9 + j] = -(K9[r][j] + K9[r][3 + j] + K9[r][6 + j])
            K[9 + j][r] = -(K9[j][r] + K9[3 + j][r] + K9[6 + j][r])
    for j in range(3):
        for j2 in range(3):
            s = xp.num(0)
            for a in range(3):
                for b in range(3):
                    s = s + K9[a * 3 + j][b * 3 + j2]
            K[9 + j][9 + j2] = s
    return K


def element_matrix(xp, x, B, W, mat, spd=0):
    K9 = block9(xp, x, B, W, mat)
    if clamps(mat, spd):
        K9 = project9(xp, K9)
    return block12(xp, K9)


def elastic_force(grad, mass, gravity, f_ext):
    """Elastic.get_force: -(gradient) + m g + f_ext, per vertex (arrays (n, 3), any scalar type)"""
    return -grad + mass[:, None] * gravity + f_ext


def mask_matrix(A, frozen, mdt2):
    """the engine's frozen rule on a dense matrix (object or float): rows / columns of frozen dofs removed, their diagonal = m / dt^2"""
    A = A.copy()
    for d in np.nonzero(np.asarray(frozen).ravel())[0]:
        A[d, :] = 0 * A[d, :]
        A[:, d] = 0 * A[:, d]
        A[d, d] = mdt2[d // 3]
    return A


def rotate(x, R):
    return np.asarray(x) @ np.asarray(R).T


# ------------------------------------------------------------------------------------------------ arrays out, relabelings, bounds
def _arr(v):
    return np.array(v, dtype=object)


def fro(a):
    a = np.asarray(a, dtype=object).ravel()
    s = 0
    for v in a:
        s = s + v * v
    return mp.sqrt(s)


PERMS = list(itertools.permutations(range(3)))


def relabel(x, B, p):
    """vertices 0..2 renumbered: new vertex k is old vertex p[k] (columns of Ds permuted = rows of B permuted)"""
    x = np.asarray(x).reshape(4, 3)
    B = np.asarray(B).reshape(3, 3)
    return x[[p[0], p[1], p[2], 3]], B[list(p)].reshape(9)


def _unlabel(v, p):
    """a 12-vector or 12 x 12 matrix computed on the relabelled element, back in the original vertex order"""
    idx = np.zeros(12, int)
    for k in range(3):
        idx[3 * p[k]:3 * p[k] + 3] = 3 * k + np.arange(3)
    idx[9:] = 9 + np.arange(3)
    v = np.asarray(v, dtype=object)
    return v[idx] if v.ndim == 1 else v[np.ix_(idx, idx)]


@with_mp
def e64_of(fun, x, B, ref):
    """largest Frobenius error of the float64 restatement against `ref` (mp) over the six relabelings of vertices 0..2: fun(xp, x, B) returns a
    scalar, a 12-vector or a 12 x 12 matrix in the element's vertex order"""
    worst = mp.mpf(0)
    for p in PERMS:
        xr, Br = relabel(x, B, p)
        v = fun(F64, xr, Br)
        if np.ndim(v) == 0:
            err = abs(mp.mpf(float(v)) - ref)
        else:
            v = _unlabel(v, p)
            err = fro(_arr([mp.mpf(float(t)) for t in np.asarray(v, dtype=object).ravel()]) - np.asarray(ref, dtype=object).ravel())
        worst = max(worst, err)
    return worst


def bound(e64, norm_mp, extra=0):
    """|gpu - mp|_F <= 8 max(e64 (+ extra), 4 u |mp|_F): three bits over what float64 delivers for the same formulas in another order"""
    return float(8 * max(e64 + extra, 4 * U * norm_mp))


# ------------------------------------------------------------------------------------------------ rest shapes, states, meshes
def _rot(axis, angle):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R1 = _rot((1.0, 2.0, -1.0), 0.7)
R2 = _rot((-2.0, 1.0, 3.0), -1.1)

CORNER = 0.01 * np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0, 0]])   # the regular corner tet with 1 cm edges
REST = {
    "corner": CORNER,
    "tiny": 1e-3 * CORNER,                                                       # B ~ 1e5, W ~ 1e-16
    "sliver": 0.01 * np.array([[1.0, 0, 0], [0.5, 0.8, 0], [0.3, 0.4, 1e-3], [0, 0, 0]]),   # cond(B) ~ 1e3
}

STATES = {   # s of A = R1 diag(s) R2
    "a": (1, 1, 1), "b": (1, 1, 0.5), "c": (3, 0.7, 1.2), "d": (10, 10, 10), "e": (1, 1, 1e-3), "f": (1, 1, 0), "g": (1, 1, -0.5),
    "h+": (1, 1, 0.0101), "h-": (1, 1, 0.0099), "i": (1, 1, -0.5),
}
STATES_OF_KIND = {0: ["a", "b", "c", "d", "e", "f", "g"], 1: ["a", "b", "c", "d", "h+", "h-", "i"]}


def rest_tables(X):
    """B (9 doubles, row major) and W of a rest tet (4, 3)"""
    Ds = np.stack([X[0] - X[3], X[1] - X[3], X[2] - X[3]], axis=1)
    return np.linalg.inv(Ds).reshape(9), abs(np.linalg.det(Ds)) / 6


def deformed(X, state, t=(0.0, 0.0, 0.0)):
    """x = A X + t; state f leaves R1 out, so that every vertex has z = 0 exactly: vertex 3 lies in the plane of the others and J = 0"""
    s = np.array(STATES[state], float)
    A = (np.diag(s) if state == "f" else R1 @ np.diag(s)) @ R2
    return X @ A.T + np.asarray(t, float)


def disjoint_mesh(items):
    """items: list of (rest name, state name): one tet each, four vertices of its own.  Returns (X rest (4 n, 3), x (4 n, 3), tets (n, 4), B, W)"""
    X = np.concatenate([REST[r] for r, _ in items])
    x = np.concatenate([deformed(REST[r], s) for r, s in items])
    tets = np.arange(4 * len(items), dtype=np.int32).reshape(-1, 4)
    BW = [rest_tables(REST[r]) for r, _ in items]
    return X, x, tets, np.array([b for b, _ in BW]), np.array([w for _, w in BW])


def cycle_items(n, kind, start=0):
    """n (rest, state) pairs: neighbours differ in both, the pattern repeats after 21 tets (not after a group of 4 or a wave of 16)"""
    rests, states = list(REST), STATES_OF_KIND[kind]
    return [(rests[(start + t) % 3], states[(start + t) % 7]) for t in range(n)]


def ring_mesh(n=24, radius=0.01, height=0.012, seed=0):
    """n tets around the shared edge (v0, v1): the two axis vertices have valence n.  x = an affine map (J = 0.6) of the rest pose plus noise
    of 5 % of the radius"""
    th = 2 * np.pi * np.arange(n) / n
    X = np.concatenate([[[0, 0, 0], [0, 0, height]], np.stack([radius * np.cos(th), radius * np.sin(th), np.full(n, height / 2)], 1)])
    tets = np.array([[0, 1, 2 + k, 2 + (k + 1) % n] for k in range(n)], np.int32)
    A = R1 @ np.diag([1.2, 1.0, 0.5]) @ R2
    x = X @ A.T + np.random.default_rng(seed).normal(scale=0.05 * radius, size=X.shape)
    BW = [rest_tables(X[t]) for t in tets]
    return X, x, tets, np.array([b for b, _ in BW]), np.array([w for _, w in BW])


def tet_context(bodies, n_verts, mass=1e-30, dt=5e-3, frozen=None):
    """engine context of elastic bodies only: bodies = list of (Material, tets (global ids), B, W, v_offset, n_verts); no cloth, no faces, no pairs,
    gravity 0.  mass: m / dt^2 stays below u times the smallest block diagonal of these meshes (1e-2 for the 1e-5 m tet), so the blocks read
    straight out of the matrix; the references add the mass term all the same"""
    from thinshelllab_amd.context import TslContext
    els = [dict(kind=m.kind, n_verts=nv, n_cells=len(t), v_offset=off, mu=m.mu, lam=m.lam, alpha=m.alpha, tets=np.asarray(t, np.int32) - off,
                B=np.asarray(B).reshape(-1, 9), W=np.asarray(W)) for m, t, B, W, off, nv in bodies]
    return TslContext(tot_NV=n_verts, dt=dt, mass=np.full(n_verts, mass), gravity=np.zeros((n_verts, 3)),
                      frozen=np.zeros(3 * n_verts, np.int32) if frozen is None else frozen, elastics=els)


# ------------------------------------------------------------------------------------------------ references of the test elements, computed once
MATERIALS = {0: Material(0, 2.0e4, 3.0e4), 1: Material(1, 1.5e4, 2.5e4)}


def _f(v):
    return np.array([float(t) for t in np.asarray(v, dtype=object).ravel()]).reshape(np.shape(v))


@functools.lru_cache(maxsize=None)
def element_reference(rest, state, kind):
    """mp values of one test element and the float64 errors e64 that go into bound(): dict with x, B, W, and per quantity q in
    energy / grad / block (unprojected 12 x 12) / block_spd (projected, where anything projects it) / dmu / dlam:
    q (mp, object array or mpf), q + "_f" (rounded to double), q + "_n" (Frobenius norm), q + "_e64"."""
    with mp.workdps(50):
        return _element_reference(REST[rest], deformed(REST[rest], state), MATERIALS[kind])


def _element_reference(X, x, mat, B=None, W=None):
    if B is None:
        B, W = rest_tables(X)
    out = dict(x=x, B=B, W=W, mat=mat)
    funs = dict(energy=lambda xp, x, B: energy(xp, x, B, W, mat),
                grad=lambda xp, x, B: gradient(xp, x, B, W, mat),
                block=lambda xp, x, B: element_matrix(xp, x, B, W, mat, 0),
                dmu=lambda xp, x, B: dgrad_dparam(xp, x, B, W, mat, "mu"),
                dlam=lambda xp, x, B: dgrad_dparam(xp, x, B, W, mat, "lam"))
    for q, fun in funs.items():
        v = fun(MP, x, B)
        ref = v if q == "energy" else _arr(v)
        out[q] = ref
        out[q + "_f"] = float(ref) if q == "energy" else _f(ref)
        out[q + "_n"] = abs(ref) if q == "energy" else fro(ref)
        out[q + "_e64"] = e64_of(fun, x, B, ref)
    K9 = [[out["block"][i, j] for j in range(9)] for i in range(9)]
    P = _arr(block12(MP, project9(MP, K9)))
    out["block_spd"], out["block_spd_f"], out["block_spd_n"] = P, _f(P), fro(P)
    S = np.array([[float((K9[i][j] + K9[j][i]) / 2) for j in range(9)] for i in range(9)])
    out["min_eig"] = float(np.linalg.eigvalsh(S).min())
    return out


def block_bound(r, projected):
    """bound() of an element's 12 x 12 block; a projected block takes e64 of the unprojected one plus 64 u |block|_F (the projection onto the PSD
    cone is non-expansive in the Frobenius norm, Jacobi stops at off^2 <= 1e-32 |A|^2)"""
    if projected:
        return bound(r["block_e64"], r["block_spd_n"], 64 * U * r["block_n"])
    return bound(r["block_e64"], r["block_n"])


# ------------------------------------------------------------------------------------------------ the meshes of the GPU tests
SIZES = (1, 3, 4, 5, 15, 16, 17, 33)   # group edges at 4, wave edges at 16; the tail groups of the last workgroup re-read tet n - 1
WARM_SEQUENCE = ("a", "g", "a", "e")


def gpu_meshes():
    """{name: [(kind, [(rest, state), ...]) per body]} of the disjoint-tet meshes (the ring has no table: ring_mesh)"""
    out = {}
    for n in SIZES:
        for kind in (0, 1):
            out["n%d_kind%d" % (n, kind)] = [(kind, cycle_items(n, kind, start=n))]
    out["two_bodies"] = [(0, cycle_items(5, 0, start=1)), (1, cycle_items(5, 1, start=4))]
    rests = list(REST)
    for k in range(4):   # tet t of the warm-start test is at state WARM_SEQUENCE[(k + t) % 4] in assembly k: every move is a large jump
        out["warm%d" % k] = [(0, [(rests[t % 3], WARM_SEQUENCE[(k + t) % 4]) for t in range(17)])]
    return out


@functools.lru_cache(maxsize=None)
def ring_reference(kind):
    X, x, tets, B, W = ring_mesh()
    with mp.workdps(50):
        return X, x, tets, B, W, [_element_reference(X[t], x[t], MATERIALS[kind], B[k], W[k]) for k, t in enumerate(tets)]
