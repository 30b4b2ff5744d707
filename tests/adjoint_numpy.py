"""Restatement of the reverse step's own kernels (csrc/k_adjoint.hpp: k_clamp, k_adj_a2ax with the hinge range of k_vertex_gather behind it, k_adj_x2a,
k_zfrozen_gather + k_scatter_perm, k_adj_prev; the halves adjoint_pre / adjoint_post of csrc/adjoint_api.hpp) for tests/test_adjoint_numpy.py and
tests/test_gpu_adjoint_elements.py, written from the reference's formulas, not from the kernels and not from oracle/:
- engine/analytic_grad_single.py:217-257 (Grad.transfer_grad): the order clamp, a2ax, un-projected Hessian at (x_s, ref_{s-1}), solve, tmp_z_frozen, x2a,
  inertia into the rows s - 1 (step > 0) and s - 2 (step > 1);
- :176-185 (clamp_grad): pos_grad[s] and angleref_grad[s] clipped at +-1000 (the engine's adj_clamp / adj_clamp_angleref make the first limit and the
  second clip switches: the system-identification class clips pos_grad at 1 and angleref_grad not at all);
- :56-60 (get_F): the right-hand side is pos_grad[s] WHOLE, frozen dofs included;
- :81-106 (get_grad, get_prev_grad, get_prev_prev_grad): x_hat_grad = p m / dt^2, pos_grad[s - 1] += (1 + d) x_hat_grad and pos_grad[s - 2] -= d x_hat_grad
  on the free dofs;
- engine/model_fold_offset.py:1180-1206 (ref_angle_backprop_a2ax): per hinge (counter_face > own face) angleref_grad[s - 1] += a, a = angleref_grad[s]
  (clipped), and pos_grad[s] of its four vertices += sgn d(theta)/dx, sgn = a where |theta - ref| > k_angle, else a * 0.1 (the double 0.1);
- :1155-1168 (ref_angle_backprop_x2a): angleref_grad[s - 1] += -(p . d(theta)/dx) d_ref over the four vertices, d_ref = -2 Kb dx^2 / 3 (:1151-1152);
  p is read at all four vertices, frozen or not;
- engine/BaseScene.py:403 (add_H under counting_z_frozen): an entry v of row i, column j with j frozen and i free gives tmp_z_frozen[j] -= v p[i].  So
  on a frozen dof (v, c) tmp_z_frozen = -sum over the free dofs (u, j) of H[(u, j)][(v, c)] p[u, j]: COLUMN (v, c) of the un-projected, un-masked
  operator.  The operator is not symmetric (the doubled term of the area block, the second-order bending part), so row and column differ; the element
  blocks of the two tetrahedron materials are symmetric, also below the clamp of J: a body alone cannot show a missing transposition.
The element formulas are not restated here: theta and d(theta)/dx come from cloth_numpy.evaluate, the operator from cloth_numpy.expected(ref, "all", 0,
()) and from the tet_numpy element blocks.

p on frozen dofs.  The right-hand side is not masked (get_F) and the engine's masked operator carries m / dt^2 on the diagonal of a frozen dof with its
row and column removed (the frozen rule of tet_numpy / cloth_numpy), so there p = pos_grad[s] (after clamp and a2ax) / (m / dt^2).  The reference's own
masked operator carries NOTHING on a frozen diagonal (add_H drops every entry of a frozen row or column, the mass term included) and its sparse solve of
that singular system is whatever the library makes of it; the engine's value is the one the oracle parity tests hold (oracle/ puts m / dt^2 there too).
p there matters to x2a alone: tmp_z_frozen and the inertia rows read free dofs only.

m / dt^2.  reverse_context() takes dt = 2^-8 and masses that are powers of two, so that m / dt^2 = MDT2 = 2^29 is a power of two and p m / dt^2, p itself
and p on the frozen dofs are exact in float64.  2^29 is the smallest power of two at which the un-projected operator of every state of GPU_STATES is
positive definite (the 3 x 2 sheet of 1e-4 m cells compressed to half puts -3.1e8 into it; tests/test_adjoint_numpy.py asserts 2^29 and that 2^28 fails).

Bounds (tet_numpy.bound): 8 max(e64, 4 u |mp|) per hinge term (sgn d(theta)/dx of one vertex; the x2a term of a hinge) and per vertex-pair block of the
operator times |p|; e64 over the evaluations of cloth_numpy.Reference (the state, its six rotations, eight one-ulp jitters, the two cosine moves).  A
per-vertex or per-slot sum takes the mp sum and the sum of its terms' bounds; terms that are exact in float64 (a clipped seed, a seed, p m / dt^2 and its
products by a power-of-two d) enter with e64 = 0.  The a2ax decision is recorded with its normalised distance from the threshold, |theta - ref| / k_angle
- 1, as cloth_numpy.update_ref records `plastic`; decisions_safe() asserts it and every decision of cloth_numpy at least cloth_numpy.SAFE away, on the
same side in mp and in every float64 evaluation."""
import functools

import mpmath as mp
import numpy as np

import cloth_numpy as cn
import tet_numpy as tn
from tet_numpy import F64, MP, U  # noqa: F401

DT = 2.0 ** -8
MDT2 = 2.0 ** 29
MASS = MDT2 * DT ** 2
ANGLEREF_CLAMP = 1000.0
TENTH = 0.1


# ------------------------------------------------------------------------------------------------ states
def _with_second(name, dx, kind, arg, ref):
    return cn._state(name, 8, 8, cn.DXS[dx], kind, arg, ref, second=(3, 2))


def _compress_rot(name, N, M, dx, second=None):
    """the sheet compressed to half and turned by R1: on a flat sheet in a coordinate plane the doubled term of the area block (the one entry that makes
    the operator differ from its transpose) meets a zero factor, and cloth_numpy's `compress` is such a sheet; its `stretch` is turned already"""
    c = cn.ClothTables(N, M, cn.DXS[dx])
    parts = [(c, cn.flat(c, 0.5, 0.5), np.zeros((c.NF, 3)), tn.R1, (0.0, 0.0, 0.0))]
    if second:
        c2, geo2, ra2, R2_ = cn._second(second[0], second[1], cn.DXS[dx], c.NV)
        parts.append((c2, geo2, ra2, R2_, (0.0, 0.0, 20 * cn.DXS[dx])))
    return cn.make_state(name, parts)


STATES = {   # the states that cloth_numpy.STATES lacks: turned compressed sheets, and 8 x 8 with a 3 x 2 second cloth (own dx, Kb, k_angle, v_offset, face_start)
    "8x8+3x2/dx1e-4/fold+90_ref0": functools.partial(_with_second, "8x8+3x2/dx1e-4/fold+90_ref0", "dx1e-4", "fold", np.pi / 2, "0"),
}
for _mesh, _dx, _second in (("1x1", "dx150", None), ("3x2", "dx150", None), ("3x2", "dx1e-4", None), ("8x8", "dx150", None), ("8x8", "dx150", (3, 2))):
    _key = "%s%s/%s/compress_rot" % (_mesh, "+3x2" if _second else "", _dx)
    STATES[_key] = functools.partial(_compress_rot, _key, int(_mesh.split("x")[0]), int(_mesh.split("x")[1]), _dx, _second)


def state(key):
    return (cn.STATES[key] if key in cn.STATES else STATES[key])()


@functools.lru_cache(maxsize=None)
def _own_reference(key):
    return cn.Reference(STATES[key]())


def reference(key):
    return cn.reference(key) if key in cn.STATES else _own_reference(key)


_FOLDS = ["fold%s%s_ref%s" % (sg, fn, rf) for fn in cn.FOLDS for sg in "+-" for rf in ("0", "same", "opp")]
SMALL_STATES = (["1x1/dx150/fold+90_refsame", "1x1/dx1e-4/stretch", "1x1/dx150/compress", "1x1/dx150/compress_rot"]
                + ["3x2/dx150/" + s for s in ["ripple1.3e-3", "ripple1.5e-3", "stretch", "compress", "compress_rot"] + _FOLDS]
                + ["3x2/dx1e-4/" + s for s in ["ripple1.3e-3", "ripple1.5e-3", "stretch", "compress", "compress_rot", "fold+pi_refopp", "fold-170_refsame",
                                               "fold-90_ref0"]])
LARGE_STATES = ["8x8/dx150/compress_rot", "8x8/dx1e-4/bump", "10x10/dx150/fold+90_ref0", "10x10/dx1e-4/ripple1.5e-3", "8x8+3x2/dx150/compress_rot",
                "8x8+3x2/dx1e-4/fold+90_ref0"]
# the area term far from rest and the sheet turned: some frozen / free block differs from its transpose by 2e-3 .. 1.7 of itself (the stretched sheets of
# 1e-4 m cells and the stretched 1 x 1 reach 2e-5 .. 6e-5 only and are ordinary states)
TRANSPOSE_STATES = [k for k in SMALL_STATES + LARGE_STATES if "compress_rot" in k] + ["3x2/dx150/stretch"]
GPU_STATES = SMALL_STATES + LARGE_STATES + list(cn.PLASTIC_KEYS)
TET_STATES = {0: "e", 1: "h-"}   # crushed to 1e-3 (kind 0), just below the clamp of J, where the literal block is no derivative any more (kind 1)


# ------------------------------------------------------------------------------------------------ frozen patterns, per dof
_CYCLE = (7, 5, 3, 0, 1, 6, 0, 2, 4, 0)


def frozen_pattern(nv, name):
    """(3 nv,) int32.  "A": vertex v takes the mask _CYCLE[v % 10] (bit c = dof c frozen): every value 1..7 from nine vertices on, vertex 0 whole next
    to the partly frozen vertex 1, vertices 1 and 2 both partly frozen; "B": the same cycle moved by one vertex, so that every vertex that A leaves
    free has a frozen dof in B (every SELL-64 slice, the partly filled last one too, then holds a frozen row in one of the two runs; a full slice
    holds one in both: 64 rows against 3 free vertices in 10); "small": the masks 7, 5, 3, 0 on four vertices; "none" """
    m = np.zeros(nv, int)
    if name == "A":
        m = np.array([_CYCLE[v % 10] for v in range(nv)])
    elif name == "B":
        m = np.array([_CYCLE[(v + 1) % 10] for v in range(nv)])
    elif name == "small":
        m[:4] = (7, 5, 3, 0)
    else:
        assert name == "none"
    return np.array([(m[v] >> c) & 1 for v in range(nv) for c in range(3)], np.int32)


def masks(frozen):
    f = np.asarray(frozen).reshape(-1, 3)
    return f[:, 0] + 2 * f[:, 1] + 4 * f[:, 2]


def pattern_properties(frozen, pattern):
    """what a frozen pattern exercises on a matrix pattern (nv, nv): the set of mask values, whether two coupled vertices are both partly frozen, whether
    a whole vertex is coupled to a partly frozen one"""
    m = masks(frozen)
    part = (m > 0) & (m < 7)
    off = pattern & ~np.eye(len(m), dtype=bool)
    return dict(values=set(m[m > 0].tolist()), both_partial=bool((off & part[:, None] & part[None, :]).any()),
                whole_next_to_partial=bool((off & (m == 7)[:, None] & part[None, :]).any()))


# ------------------------------------------------------------------------------------------------ the engine context
def reverse_context(cloths, nv, frozen=None, mdt2=MDT2, bodies=()):
    """engine context of cloths (and elastic bodies: tuples as tet_numpy.tet_context takes them), no faces table, no pairs, gravity 0, dt = 2^-8 and every
    mass mdt2 dt^2: powers of two"""
    from thinshelllab_amd.context import TslContext
    els = [dict(kind=m.kind, n_verts=n, n_cells=len(t), v_offset=off, mu=m.mu, lam=m.lam, alpha=m.alpha, tets=np.asarray(t, np.int32) - off,
                B=np.asarray(B).reshape(-1, 9), W=np.asarray(W)) for m, t, B, W, off, n in bodies]
    return TslContext(tot_NV=nv, dt=DT, mass=np.full(nv, mdt2 * DT ** 2), gravity=np.zeros((nv, 3)),
                      frozen=np.zeros(3 * nv, np.int32) if frozen is None else frozen, cloths=[c.desc for c in cloths], elastics=els)


# ------------------------------------------------------------------------------------------------ the operator
class Operator:
    """the un-projected, un-masked operator as mp (hi, lo) halves of a dense (3 nv, 3 nv) matrix [row][column] (without a mass term worth the name: the
    cloth part carries cloth_numpy's 1e-30 / dt^2 on its diagonal, which no quantity here reads), the bound Ab (nv, nv) per vertex-pair block, the
    pattern (nv, nv), and f64: function k -> the same matrix from the k-th float64 evaluation (None where the CPU harness does not go)"""
    def __init__(self, hl, Ab, pattern, f64=None):
        self.hl, self.Ab, self.pattern, self.f64, self.nv = hl, Ab, pattern, f64, len(Ab)

    def dense(self, mdt2):
        """float64 rounding of the mp operator with mdt2 on the diagonal"""
        return self.hl[0] + mdt2 * np.eye(3 * self.nv)


@functools.lru_cache(maxsize=None)
def cloth_operator(ref):
    e = cn.expected(ref, "all", 0, ())
    return Operator(e.A, e.Ab, e.pattern, lambda k: cn.f64_assembly(ref, "all", k)[0])


@functools.lru_cache(maxsize=None)
def ring(kind):
    """one tet_numpy.ring_mesh body of material `kind` in the crushed state TET_STATES[kind]: (x, tets, B, W, mp element blocks, their bounds)"""
    X, _, tets, B, W = tn.ring_mesh()
    x = tn.deformed(X, TET_STATES[kind])
    mat = tn.MATERIALS[kind]
    blocks, bnds = [], []
    with mp.workdps(50):
        for k, t in enumerate(tets):
            fun = lambda xp, xx, BB, w=W[k]: tn.element_matrix(xp, xx, BB, w, mat, 0)   # noqa: E731
            blk = tn._arr(fun(MP, x[t], B[k]))
            blocks.append(blk)
            bnds.append(tn.bound(tn.e64_of(fun, x[t], B[k], blk), tn.fro(blk)))
    return x, tets, B, W, blocks, bnds


def tet_operator(kind, nv=None, off=0):
    """the ring body's operator on vertices off .. off + 26 of nv: sum of the element blocks, a vertex pair's bound the sum of its elements' block bounds"""
    x, tets, _, _, blocks, bnds = ring(kind)
    n = len(x)
    nv = n if nv is None else nv
    with mp.workdps(50):
        A = np.full((3 * nv, 3 * nv), mp.mpf(0), dtype=object)
        Ab, pat = np.zeros((nv, nv)), np.zeros((nv, nv), bool)
        for t, blk, b in zip(tets + off, blocks, bnds):
            d = (3 * np.asarray(t)[:, None] + np.arange(3)).ravel()
            A[np.ix_(d, d)] += blk
            Ab[np.ix_(t, t)] += b
            pat[np.ix_(t, t)] = True
        return Operator(cn.split(A), Ab, pat)


def join(a, b):
    """two operators on the same vertices without a common entry (a cloth and a body), summed"""
    return Operator((a.hl[0] + b.hl[0], a.hl[1] + b.hl[1]), a.Ab + b.Ab, a.pattern | b.pattern)


def pad(op, nv):
    """an operator on the first vertices of nv"""
    n = op.nv
    hl = [np.zeros((3 * nv, 3 * nv)), np.zeros((3 * nv, 3 * nv))]
    for k in (0, 1):
        hl[k][:3 * n, :3 * n] = op.hl[k]
    Ab, pat = np.zeros((nv, nv)), np.zeros((nv, nv), bool)
    Ab[:n, :n], pat[:n, :n] = op.Ab, op.pattern
    return Operator(tuple(hl), Ab, pat)


def min_eigenvalue(op, mdt2):
    A = op.dense(mdt2)
    return float(np.linalg.eigvalsh(0.5 * (A + A.T)).min())


# ------------------------------------------------------------------------------------------------ hinges of a state
def hinge_layout(st):
    """[(cloth i, hinge h of cloth_numpy's order, slot 3 (face_start + f) + l of a row of angleref_grad / ref_buffer, the four global vertices)]"""
    out, f0 = [], 0
    for i, c in enumerate(st.cloths):
        for h, (f, l) in enumerate(c.hinges):
            out.append((i, h, 3 * (f0 + f) + l, np.array(c.hinge_verts(f, l)[0]) + c.v_offset))
        f0 += c.NF
    return out


def n_slots(st):
    return 3 * max(sum(c.NF for c in st.cloths), 1)


def ref_row(st):
    """the row ref_{s-1} of the tape"""
    return np.concatenate(st.ra).ravel() if st.cloths else np.zeros(3)


def a2ax_sign(xp, theta, ra, k_angle, a, dec=None):
    """:1191-1201: a where |theta - ref| > k_angle, else a * 0.1"""
    dis, ka = abs(theta - xp.num(ra)), xp.num(k_angle)
    if dec is not None:
        dec.append(("a2ax", dis / ka - 1))
    return xp.num(a) if dis > ka else xp.num(a) * xp.num(TENTH)


def d_ref(xp, c):
    """:1151-1152"""
    return xp.num(-2.0) * xp.num(c.Kb) * xp.num(c.dx) ** 2 / xp.num(3.0)


def x2a_term(xp, g, pv, dr):
    """:1162-1168 for one hinge: -(sum over the four vertices of p . d(theta)/dx) d_ref"""
    s = xp.num(0)
    for a in range(4):
        for j in range(3):
            s = s + xp.num(pv[a][j]) * g[a][j]
    return -s * dr


def decisions_safe(ref):
    """cloth_numpy.decisions_safe of the state, and the a2ax decision of every hinge at least SAFE from its threshold on the same side in mp and in every
    float64 evaluation the bounds are taken from"""
    st = ref.st
    assert cn.decisions_safe(st)
    ra = ref_row(st)
    with mp.workdps(50):
        for i, h, slot, _ in hinge_layout(st):
            ka = st.cloths[i].k_angle
            dm = float(abs(ref.mp[i]["theta"][h] - mp.mpf(float(ra[slot]))) / mp.mpf(ka) - 1)
            assert abs(dm) >= cn.SAFE, (st.name, i, h, dm)
            for ev in ref.f64[i]:
                df = abs(ev["theta"][h] - ra[slot]) / ka - 1
                assert abs(df) >= cn.SAFE and (df > 0) == (dm > 0), (st.name, i, h, dm, df)
    return True


# ------------------------------------------------------------------------------------------------ one step: inputs
class Inputs:
    """what one adjoint_step at step s reads beside the tape rows (x_s and ref_{s-1} are the state's; x_{s-1} decides nothing without contacts and
    colliders: the operator is assembled at x_s): the seeds pg_s (nv, 3), ag_s, ag_prev (slots,), pg_prev, pg_prev2 (nv, 3; None at s = 1), the frozen
    dofs (3 nv,), adj_clamp, the angleref switch, the damping d, m / dt^2"""
    def __init__(self, s, pg_s, ag_s, ag_prev, pg_prev, pg_prev2, frozen, adj_clamp=1000.0, clamp_angleref=1, d=1.0, mdt2=MDT2):
        assert (pg_prev2 is None) == (s == 1)
        self.s, self.pg_s, self.ag_s, self.ag_prev, self.pg_prev, self.pg_prev2 = s, pg_s, ag_s, ag_prev, pg_prev, pg_prev2
        self.frozen, self.adj_clamp, self.clamp_angleref, self.d, self.mdt2 = np.asarray(frozen).reshape(-1, 3).astype(bool), adj_clamp, clamp_angleref, d, mdt2


def clipped_angleref(st, inp):
    return np.clip(inp.ag_s, -ANGLEREF_CLAMP, ANGLEREF_CLAMP) if (inp.clamp_angleref and st.cloths) else inp.ag_s.copy()


def frozen_p(p_free, pg_s_after, inp):
    """the rule for p on frozen dofs: pos_grad[s] after clamp and a2ax over m / dt^2 there (exact: a power of two), p_free elsewhere"""
    return np.where(inp.frozen, np.asarray(pg_s_after).reshape(-1, 3) / inp.mdt2, np.asarray(p_free).reshape(-1, 3))


def _mpa(a):
    return np.array([mp.mpf(float(v)) for v in np.asarray(a).ravel()], dtype=object).reshape(np.shape(a))


def _e64(ref, i, fun, want, axis):
    """largest error (norm over the last axis where axis) of fun(float64 evaluation) against the mp array `want` over the evaluations of the Reference"""
    hi, lo = cn.split(want)
    worst = None
    for ev in ref.f64[i]:
        d = (fun(ev) - hi) - lo
        n = np.sqrt((d * d).sum(axis=-1)) if axis else np.abs(d)
        worst = n if worst is None else np.fmax(worst, n)
    return worst


def _a2ax64(ev, sgn64):
    return sgn64[:, None, None] * ev["g"]


def _x2a64(ev, c, hv, p):
    dr = d_ref(F64, c)
    return np.array([x2a_term(F64, ev["g"][h], p[hv[h]], dr) for h in range(len(hv))])


# ------------------------------------------------------------------------------------------------ one step: what it must write
def expected_reverse(ref, op, inp, p, st=None):
    """mp values and bounds of everything one adjoint_step writes, for the complete vector p (nv, 3) (frozen_p).  ref: the Reference of the state (x_s,
    ref_{s-1}), None without a cloth (then st = None too and op spans the vertices); op: the Operator.  Returns a dict:
    pg_s, tz, pg_prev, pg_prev2 (None at s = 1): ((hi, lo) (nv, 3), bound (nv,) on the vertex's 2-norm); clip: the clipped seed (nv, 3) and quiet (nv,):
    vertices whose hinges all carry a == 0 (pos_grad[s] == clip bit for bit there); ag_s: the exact row; ag_prev: ((hi, lo), bound) per slot and
    touched (slots,): every other slot keeps its bits; x2a: ((hi, lo), bound) per slot of the x2a term alone; far: {slot: took the `> k_angle`
    branch}; dec: the a2ax decisions"""
    st = ref.st if ref is not None else st
    nv = op.nv
    lay = hinge_layout(st) if st is not None else []
    out = {}
    with mp.workdps(50):
        zero = mp.mpf(0)
        ag_s = clipped_angleref(st, inp) if st is not None else inp.ag_s.copy()
        clip = np.clip(inp.pg_s, -inp.adj_clamp, inp.adj_clamp)
        pg = _mpa(clip)
        pgb = 32 * U * np.sqrt((clip ** 2).sum(axis=1))
        quiet = np.ones(nv, bool)
        agp = _mpa(inp.ag_prev)
        agb = 32 * U * np.abs(inp.ag_prev)
        touched = np.zeros(len(inp.ag_prev), bool)
        x2a, x2ab = np.full(len(inp.ag_prev), zero, dtype=object), np.zeros(len(inp.ag_prev))
        far, dec = {}, []
        ra = ref_row(st) if st is not None else None
        for i, c in enumerate(st.cloths if st is not None else []):
            mine = [(h, slot, hv) for ci, h, slot, hv in lay if ci == i]
            if not mine:
                continue
            slots, hv = np.array([t[1] for t in mine]), np.array([t[2] for t in mine])
            sgn, sgn64 = [], []
            for h, slot, _ in mine:
                a = ag_s[slot]
                sgn.append(a2ax_sign(MP, ref.mp[i]["theta"][h], ra[slot], c.k_angle, a, dec))
                far[slot] = dec[-1][1] > 0
                sgn64.append(np.float64(a) if far[slot] else np.float64(a) * np.float64(TENTH))
            term = np.array(sgn, dtype=object)[:, None, None] * ref.mp[i]["g"]
            e = _e64(ref, i, lambda ev: _a2ax64(ev, np.array(sgn64)), term, True)
            tb = cn._bnd(e, np.sqrt((cn.split(term)[0] ** 2).sum(axis=-1)))
            for k in range(len(mine)):
                a = ag_s[slots[k]]
                for j in range(4):
                    pg[hv[k, j]] += term[k, j]
                    pgb[hv[k, j]] += tb[k, j]
                    if a != 0:
                        quiet[hv[k, j]] = False
            dr = d_ref(MP, c)
            pm = _mpa(p)
            xt = np.array([x2a_term(MP, ref.mp[i]["g"][h], pm[hv[k]], dr) for k, (h, _, _) in enumerate(mine)], dtype=object)
            xe = _e64(ref, i, lambda ev: _x2a64(ev, c, hv, p), xt, False)
            xb = cn._bnd(xe, np.abs(cn.split(xt)[0]))
            for k in range(len(mine)):
                a = ag_s[slots[k]]
                agp[slots[k]] += mp.mpf(float(a)) + xt[k]
                agb[slots[k]] += 32 * U * abs(a) + xb[k]
                x2a[slots[k]], x2ab[slots[k]] = xt[k], xb[k]
                touched[slots[k]] = True
        out.update(pg_s=(cn.split(pg), pgb), clip=clip, quiet=quiet, ag_s=ag_s, ag_prev=(cn.split(agp), agb), touched=touched,
                   x2a=(cn.split(x2a), x2ab), far=far, dec=dec)
        # tmp_z_frozen: column (v, c) of the operator against p on the free dofs
        fz = inp.frozen
        tz = np.full((nv, 3), zero, dtype=object); tzb = np.zeros(nv)
        pf = np.where(fz, 0.0, p)
        for v in np.nonzero(fz.any(axis=1))[0]:
            for u in np.nonzero(op.pattern[:, v])[0]:
                if fz[u].all():
                    continue
                for cc in np.nonzero(fz[v])[0]:
                    for j in np.nonzero(~fz[u])[0]:
                        tz[v, cc] -= (mp.mpf(op.hl[0][3 * u + j, 3 * v + cc]) + mp.mpf(op.hl[1][3 * u + j, 3 * v + cc])) * mp.mpf(float(p[u, j]))
                tzb[v] += op.Ab[u, v] * np.sqrt((pf[u] ** 2).sum())
        out["tz"] = (cn.split(tz), tzb)
        # inertia: x_hat_grad = p m / dt^2 on the free dofs (exact), (1 + d) and d in mp
        xh = _mpa(pf * inp.mdt2)
        dm = mp.mpf(float(inp.d))
        t1 = (1 + dm) * xh
        out["pg_prev"] = (cn.split(_mpa(inp.pg_prev) + t1), 32 * U * (np.sqrt((inp.pg_prev ** 2).sum(axis=1)) + np.sqrt((cn.split(t1)[0] ** 2).sum(axis=1))))
        out["pg_prev2"] = None
        if inp.s > 1:
            t2 = dm * xh
            out["pg_prev2"] = (cn.split(_mpa(inp.pg_prev2) - t2),
                               32 * U * (np.sqrt((inp.pg_prev2 ** 2).sum(axis=1)) + np.sqrt((cn.split(t2)[0] ** 2).sum(axis=1))))
    return out


# ------------------------------------------------------------------------------------------------ comparing a step's outputs
def compare(exp, got, R, tag="", frozen=None):
    """got: dict with pg_s, ag_s, ag_prev, tz, pg_prev, pg_prev2 (float arrays) -> largest error / bound per quantity into the Ratios R; the exact parts
    (angleref_grad[s], untouched slots, quiet vertices, zeros of tmp_z_frozen on free dofs) are asserted after every ratio has been entered"""
    exact = []

    def diff(g, hl):   # (cloth_numpy.diff that keeps the extra digits of the float64 stand-in's extended sums; the same for float64 input)
        return np.asarray((np.asarray(g, np.longdouble) - hl[0]) - hl[1], float)

    def per_vertex(q, name):
        (hl, bnd), g = exp[q], np.asarray(got[q]).reshape(-1, 3)
        err = np.sqrt((diff(g, hl) ** 2).sum(axis=1))
        on = bnd > 0
        if err[~on].any():
            exact.append(name + ": exact where the bound is zero")
        if on.any():
            R.add(name + tag, float((err[on] / bnd[on]).max()), 1.0)
    per_vertex("pg_s", "pos_grad[s]")
    g = np.asarray(got["pg_s"]).reshape(-1, 3)
    if not np.array_equal(np.asarray(g, float)[exp["quiet"]], exp["clip"][exp["quiet"]]):
        exact.append("pos_grad[s] == clip(seed) where no hinge carries a gradient")
    if not np.array_equal(got["ag_s"], exp["ag_s"]):
        exact.append("angleref_grad[s]")
    (hl, bnd), t = exp["ag_prev"], exp["touched"]
    if not np.array_equal(np.asarray(got["ag_prev"])[~t], hl[0][~t]):
        exact.append("angleref_grad[s-1] off the hinges")
    if t.any():
        err = np.abs(diff(got["ag_prev"], hl))[t]
        zero = bnd[t] == 0
        if err[zero].any():
            exact.append("angleref_grad[s-1]: exact where the bound is zero")
        if (~zero).any():
            R.add("angleref_grad[s-1]" + tag, float((err[~zero] / bnd[t][~zero]).max()), 1.0)
    if frozen is not None and np.asarray(got["tz"]).reshape(-1, 3)[~np.asarray(frozen).reshape(-1, 3).astype(bool)].any():
        exact.append("tmp_z_frozen on free dofs")
    per_vertex("tz", "tmp_z_frozen")
    per_vertex("pg_prev", "pos_grad[s-1]")
    if exp["pg_prev2"] is not None:
        per_vertex("pg_prev2", "pos_grad[s-2]")
    assert not exact, exact


# ------------------------------------------------------------------------------------------------ float64 in the kernels' place
VARIANTS = ("no_transpose", "no_tenth", "compare", "a2ax_first", "d_for_1pd", "rm_skip", "p_zero_frozen")


def f64_step(ref, op, inp, p, k=1, variant=None):
    """the whole step in float64 from the k-th float64 evaluation of the Reference (another rotation: other rounding) and the given p; variant: one of
    the wrong kernels of tests/test_adjoint_numpy.py.  Same keys as compare() takes.  Every term is a float64 value of the float64 formulas; the sums
    over terms are carried in extended precision (np.longdouble), so that the harness measures the terms against their bounds: 1 / 8 where e64 is met.
    (A float64 sum of n terms adds up to u sum |terms|, 1 / 32 of the summed bound, which the kernels' ratios include.)"""
    ld = np.longdouble
    st = ref.st
    nv = st.nv
    ra, fz = ref_row(st), inp.frozen
    ag_s = clipped_angleref(st, inp)
    ag_prev = inp.ag_prev.astype(ld)
    first = variant == "a2ax_first"
    pg = (inp.pg_s.copy() if first else np.clip(inp.pg_s, -inp.adj_clamp, inp.adj_clamp)).astype(ld)
    pz = np.where(fz, 0.0, p) if variant == "p_zero_frozen" else p
    for i, h, slot, hv in hinge_layout(st):
        ev, c = ref.f64[i][k], st.cloths[i]
        a = ag_s[slot]
        ag_prev[slot] += a
        far = abs(ev["theta"][h] - ra[slot]) > c.k_angle
        if variant == "compare":
            far = not far
        sgn = a if (far or variant == "no_tenth") else a * TENTH
        for j in range(4):
            pg[hv[j]] += sgn * ev["g"][h, j]
    if first:
        pg = np.clip(pg, -inp.adj_clamp, inp.adj_clamp)
    for i, h, slot, hv in hinge_layout(st):
        ag_prev[slot] += x2a_term(F64, ref.f64[i][k]["g"][h], pz[hv], d_ref(F64, st.cloths[i]))
    A = op.f64(k)
    tz = np.zeros((nv, 3), ld)
    for v in np.nonzero(fz.any(axis=1))[0]:
        for u in np.nonzero(op.pattern[:, v])[0]:
            if fz[u].all() or (variant == "rm_skip" and fz[u].any()):
                continue
            for cc in np.nonzero(fz[v])[0]:
                s = ld(0)
                for j in np.nonzero(~fz[u])[0]:
                    s += ld(A[3 * v + cc, 3 * u + j] if variant == "no_transpose" else A[3 * u + j, 3 * v + cc]) * ld(p[u, j])
                tz[v, cc] -= s
    xh = np.where(fz, 0.0, p * inp.mdt2).astype(ld)
    out = dict(pg_s=pg, ag_s=ag_s, ag_prev=ag_prev, tz=tz, pg_prev=inp.pg_prev + xh * ld(inp.d if variant == "d_for_1pd" else 1.0 + inp.d), pg_prev2=None)
    if inp.s > 1:
        out["pg_prev2"] = inp.pg_prev2 - xh * ld(inp.d)
    return out


# ------------------------------------------------------------------------------------------------ seeds
def seeds(st, nv, s, frozen, adj_clamp=1000.0, clamp_angleref=1, d=1.0, seed=0, mdt2=MDT2, p_row=None, quiet_corner=True):
    """Inputs with seeds that are non-zero on frozen dofs too: pos_grad[s] normal entries of the size of the limit / 4 with entries inside, exactly at
    and beyond +-adj_clamp; angleref_grad[s] normal with entries at and beyond +-1000, and zero on every hinge of vertex 0, of the last vertex of
    the first cloth and of the last vertex (quiet_corner: pos_grad[s] == clip(seed) there bit for bit, because a == 0 makes every term +-0 whatever Kb
    and the geometry); the other rows normal.  p_row: the row that must start from zeros so that p can be read from it: "prev2" (default where s > 1
    and d != 0), "prev", or "none" (every row seeded: p comes from elsewhere)"""
    rng = np.random.default_rng(1000 * seed + nv + s)
    lim = adj_clamp
    pg_s = rng.normal(size=(nv, 3)) * lim / 4
    flat = pg_s.reshape(-1)
    pick = rng.permutation(3 * nv)[:6] if nv >= 4 else np.arange(6)
    flat[pick] = np.array([lim, -lim, 3 * lim, -2.5 * lim, np.nextafter(lim, 0), -np.nextafter(lim, np.inf)])
    ns = n_slots(st) if st is not None else 3
    ag_s, ag_prev = rng.normal(size=ns), rng.normal(size=ns)
    lay = hinge_layout(st) if st is not None else []
    corners = {0, nv - 1, st.cloths[0].NV - 1} if (quiet_corner and len(lay) >= 4) else set()
    for _, _, slot, hv in lay:
        if corners & set(hv.tolist()):
            ag_s[slot] = 0.0
    hs = [slot for _, _, slot, hv in lay if not corners & set(hv.tolist())]
    if len(hs) >= 3:
        ag_s[[hs[0], hs[-1], hs[len(hs) // 2]]] = (ANGLEREF_CLAMP, -4 * ANGLEREF_CLAMP, 2.5 * ANGLEREF_CLAMP)
    elif hs:
        ag_s[hs[0]] = -4 * ANGLEREF_CLAMP
    pg_prev, pg_prev2 = rng.normal(size=(nv, 3)), (rng.normal(size=(nv, 3)) if s > 1 else None)
    if p_row is None:
        p_row = "prev2" if (s > 1 and d != 0) else "prev"
    if p_row == "prev2":
        pg_prev2 = np.zeros((nv, 3))
    elif p_row == "prev":
        pg_prev = np.zeros((nv, 3))
    return Inputs(s, pg_s, ag_s, ag_prev, pg_prev, pg_prev2, frozen, adj_clamp, clamp_angleref, d, mdt2)
