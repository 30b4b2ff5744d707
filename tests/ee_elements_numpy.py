"""Restatement of the edge-edge contact constraint ("contact_ee" = 1; csrc/k_contact.hpp: ee_qualifies, k_ee_build, k_contact_assemble_coop<LIT, true>,
k_ee_energy, k_ee_backprop, k_contact_mask; k_contact_zfrozen_gather of csrc/k_adjoint.hpp) for tests/test_ee_elements_numpy.py and
tests/test_gpu_ee_elements.py, written from the model as DESIGN.md 2.1 and include/tsl_hip.h state it, not from the kernels.  It stands on
tests/contact_numpy.py: the backends MP (mpmath, 50 digits) and F64 (float64 scalars, the same formulas in plain order), normal_part_q (the quotient rule
for d = D / C in relative coordinates), clamp, f0 / f1 / f2, friction_core, the bound, SlotRef / Expected / check_assembly / expected_reverse, which take
this module's slot functions as their `model`.  Nothing here calls the GPU except probe_context().  The broad phase and k_ee_query are not restated: they
deliver the slots, the slots are data.

Conventions restated:
- a candidate is a query edge (a0, a1) and a target edge (b0, b1), each in ascending vertex order.  d1 = a1 - a0, d2 = b1 - b0, r = a0 - b0,
  cr = d2 x d1, cc = |cr|^2; it qualifies when cc >= 1e-4 |d1|^2 |d2|^2, s = ((d1 . d2)(d2 . r) - (d1 . r)|d2|^2) / cc and
  t = (|d1|^2 (d2 . r) - (d1 . d2)(d1 . r)) / cc lie strictly inside (0, 1), and |D| / C < eps with D = cr . r, C = sqrt(cc);
- where D < 0 the query vertices swap, s -> 1 - s, D -> -D: the slot's line distance is positive at the detection;
- idx = (b0, b1, q0, q1), w = (s, t, 0), n = (b1 - b0) x (q1 - q0) / C, gap = D / C, k = -mu k_contact (gap - eps),
  dx0 = ((1 - s) prev_q0 + s prev_q1) - ((1 - t) prev_b0 + t prev_b1), T from n as for a vertex-triangle slot (the |n.x| < 0.5 branch);
- evaluation at pos: q = (a, b, p) = (x1 - x0, x3 - x2, x2 - x0), d = D / C of contact_numpy.normal_part_q; vertex u is sum_i M[u][i] q_i with
  M = ((-1, 0, -1), (1, 0, 0), (0, -1, 1), (0, 1, 0)): gradient M g9, block M H9 M^T; spd: the 9 x 9 clamp in q-space, then the 2 x 2 clamp on the
  friction core, each before the map;
- C == 0 exactly (a x b zero bit for bit: axis-aligned edges turned parallel): D / C is 0 / 0, the comparison with eps is false, the normal part is off
  and the friction part is evaluated as usual (normal_part_q).  A rule for that one outcome, used only where the float64 restatement sees a x b == 0.0;
- friction on the lagged slip a(s) - b(t) - dx0 with w1 = (t - 1, -t, 1 - s, s);
- reverse step: contact_numpy.slot_reverse's two terms with wp = -w1; tmp_z_frozen and the frozen rule are those of contact_numpy (they work on blocks).

Decisions, each with its normalised distance from the threshold: at the detection cc >= 1e-4 aa ee ("sin"), s > 0, s < 1, t > 0, t < 1, |D| / C < eps
("gap"), the sign of D ("side", D / (C eps)), |n.x| < 0.5; at the evaluation those of contact_numpy (d < eps, r > eps_v dt, r > 1e-9)."""
import functools

import mpmath as mp
import numpy as np

import contact_numpy as cn
import ee_numpy as en
from contact_numpy import (CE_FACTOR, DT, EH, EPS, EPS_V, F64, GRID_H, K_CONTACT, MP, MU_CC, MU_CE, MU_FIXED, R_GUARD, SAFE, SC, U,  # noqa: F401
                           _P, _V, _cross, _dot, _norm, _sub, _z, diff, jitters, ratio, rotations, split)

SIN_MIN = 1e-2
M = ((-1, 0, -1), (1, 0, 0), (0, -1, 1), (0, 1, 0))


# ------------------------------------------------------------------------------------------------ records of a slot
def slot_records(xp, Xd, Pd, mu, sc=SC, dec=None):
    """Xd, Pd: (4, 3) positions and previous positions of (a0, a1, b0, b1).  None where the pair does not qualify, else dict(order, w, gap, k, mu, dx0, n, T,
    swapped): order = the slot's vertices (b0, b1, q0, q1) as positions 0..3 of the input"""
    X, P = _P(xp, Xd), _P(xp, Pd)
    note = (lambda name, v: dec.append((name, v))) if dec is not None else (lambda name, v: None)
    d1, d2, r = _sub(X[1], X[0]), _sub(X[3], X[2]), _sub(X[0], X[2])
    aa, ee, ab, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    cr = _cross(d2, d1)
    cc = _dot(cr, cr)
    thr = xp.num(SIN_MIN) * xp.num(SIN_MIN) * aa * ee
    note("sin", cc / thr - 1)
    if not cc >= thr or not cc > 0:
        return None
    s, t = (ab * f - c * ee) / cc, (aa * f - ab * c) / cc
    one = xp.num(1)
    for name, v in (("s>0", s), ("s<1", one - s), ("t>0", t), ("t<1", one - t)):
        note(name, v)
    if not (s > 0 and s < 1 and t > 0 and t < 1):
        return None
    C, D, eps = xp.sqrt(cc), _dot(cr, r), xp.num(sc.eps)
    note("gap", abs(D) / C / eps - 1)
    if not abs(D) / C < eps:
        return None
    note("side", D / C / eps)
    order, swapped = [2, 3, 0, 1], False
    if D < 0:
        order, swapped, s, D = [2, 3, 1, 0], True, one - s, -D
    q0, q1 = order[2], order[3]
    cn_ = _cross(d2, _sub(X[q1], X[q0]))
    n = [v / C for v in cn_]
    gap, mu = D / C, xp.num(mu)
    dx0 = [(P[q0][j] * (one - s) + P[q1][j] * s) - (P[2][j] * (one - t) + P[3][j] * t) for j in range(3)]
    note("nx", abs(n[0]) / xp.num(0.5) - 1)
    t1 = [n[0], n[2], -n[1]] if abs(n[0]) < xp.num(0.5) else [n[1], -n[0], n[2]]
    t2 = _cross(n, t1)
    t1 = _cross(n, t2)
    return dict(order=order, swapped=swapped, w=[s, t, xp.num(0)], gap=gap, k=-mu * (xp.num(sc.k_contact) * (gap - eps)), mu=mu, dx0=dx0, n=n, T=t1 + t2)


# ------------------------------------------------------------------------------------------------ evaluation of a slot
def to12(xp, g9, H9):
    """relative coordinates -> vertices through M: g_u = sum_i M[u][i] g9_i, H_uv = sum_ij M[u][i] M[v][j] H9_ij"""
    g = [xp.num(0)] * 12
    H = _z(xp, 12, 12)
    for u in range(4):
        for a in range(3):
            for i in range(3):
                if M[u][i]:
                    g[3 * u + a] = g[3 * u + a] + M[u][i] * g9[3 * i + a]
    for u in range(4):
        for v in range(4):
            for i in range(3):
                for j in range(3):
                    if M[u][i] and M[v][j]:
                        for a in range(3):
                            for b in range(3):
                                H[3 * u + a][3 * v + b] = H[3 * u + a][3 * v + b] + (M[u][i] * M[v][j]) * H9[3 * i + a][3 * j + b]
    return g, H


def weights(xp, w):
    s, t, one = xp.num(w[0]), xp.num(w[1]), xp.num(1)
    return s, t, [t - one, -t, one - s, s]


def friction_part(xp, X, rec, sc=SC, spd=0, dec=None):
    s, t, w1 = weights(xp, rec["w"])
    one, dx0 = xp.num(1), _V(xp, rec["dx0"])
    dx = [(X[2][j] * (one - s) + X[3][j] * s) - (X[0][j] * (one - t) + X[1][j] * t) - dx0[j] for j in range(3)]
    return cn.friction_core(xp, dx, w1, rec, sc, spd, dec)


def normal_part(xp, X, sc=SC, dec=None):
    return cn.normal_part_q(xp, _sub(X[1], X[0]), _sub(X[3], X[2]), _sub(X[2], X[0]), sc, dec)


def slot_eval(xp, X, rec, sc=SC, spd=0, dec=None):
    """energy, 12 gradient entries, 12 x 12 block of one slot at the positions X (4, 3) in the slot's order (b0, b1, q0, q1); gn1, gf1 as contact_numpy"""
    X = _P(xp, X)
    d, active, e_n, g9, H9 = normal_part(xp, X, sc, dec)
    if spd and active:
        H9 = cn.clamp(xp, H9)
    g, H = to12(xp, g9, H9)
    fr = friction_part(xp, X, rec, sc, spd, dec)
    for i1 in range(4):
        for j1 in range(3):
            g[3 * i1 + j1] = g[3 * i1 + j1] + fr["w1"][i1] * fr["g1"][j1]
            for i2 in range(4):
                for j2 in range(3):
                    H[3 * i1 + j1][3 * i2 + j2] = H[3 * i1 + j1][3 * i2 + j2] + fr["w1"][i1] * fr["w1"][i2] * fr["h1"][j1][j2]
    kc = xp.num(sc.k_contact)
    gn1 = [v / kc for v in to12(xp, g9, _z(xp, 9, 9))[0]]
    gf1 = [fr["w1"][i] * fr["tu"][j] for i in range(4) for j in range(3)]
    return dict(E=e_n + fr["e"], En=e_n, Ef=fr["e"], g=g, H=H, gn1=gn1, gf1=gf1, d=d, r=fr["r"], active=active)


def slot_reverse(xp, X, rec, z, sc=SC, wp_out=-1):
    """the 12 entries of k_ee_backprop for the 12 values z of the slot's vertices: the friction-lag term with wp = -w1 through n, k_contact and
    pressure = k / mu, plus the friction-block term; acc_lag: the first term alone.  The lag term holds wp twice, in the sum over z and on the entry it
    writes: it is the same polynomial for wp = -w1 and wp = +w1, and only a sign on ONE of the two changes it (wp_out: the sign on the written entry)"""
    X = _P(xp, X)
    fr = friction_part(xp, X, rec, sc, 0)
    n, z = _V(xp, rec["n"]), _V(xp, z)
    wp = [-v for v in fr["w1"]]
    pressure = xp.num(rec["k"]) / xp.num(rec["mu"])
    s = xp.num(0)
    for i1 in range(4):
        for j1 in range(3):
            s = s + z[3 * i1 + j1] * (wp[i1] * fr["g1"][j1] / pressure)
    lag = [s * (-wp_out * wp[i2]) * n[j2] * xp.num(sc.k_contact) for i2 in range(4) for j2 in range(3)]
    blk = [xp.num(0)] * 12
    for i1 in range(4):
        for i2 in range(4):
            for j1 in range(3):
                for j2 in range(3):
                    blk[3 * i2 + j2] = blk[3 * i2 + j2] + z[3 * i1 + j1] * fr["w1"][i1] * fr["w1"][i2] * fr["h1"][j1][j2]
    fg = [wp[i1] * fr["g1"][j1] for i1 in range(4) for j1 in range(3)]
    return dict(acc=[a + b for a, b in zip(lag, blk)], fg=fg, acc_lag=lag)


class _EdgeEdge:
    """the slot functions of this module for contact_numpy.SlotRef / Expected / f64_copies, looked up when called (a test may patch them)"""
    slot_eval = staticmethod(lambda *a, **k: slot_eval(*a, **k))
    slot_reverse = staticmethod(lambda *a, **k: {q: v for q, v in slot_reverse(*a, **k).items() if q != "acc_lag"})


EE = _EdgeEdge()


# ------------------------------------------------------------------------------------------------ probe scenes
class Probe:
    """one target triangle (b_lo, b_hi, c_b) + apex and one query triangle (a_lo, a_hi, c_a) + apex, in vertex order: tgt, qry (4, 3), their previous
    positions, the kind of mu, whether the detection must list it"""
    def __init__(self, tgt, qry, ptgt, pqry, kind, active, tag, La, Lb, s, t, swapped):
        self.tgt, self.qry, self.ptgt, self.pqry, self.kind, self.active, self.tag = tgt, qry, ptgt, pqry, kind, active, tag
        self.La, self.Lb, self.s, self.t, self.swapped = La, Lb, s, t, swapped


LS = cn.LS
NX = cn.NX
FOLD, TILT = 0.8, 0.025


def _target(center, Lb, t, n, e1, e2, fold=FOLD):
    b0 = center - t * Lb * e1
    b1 = b0 + Lb * e1
    mid = 0.5 * (b0 + b1)
    return np.array([b0, b1, mid + Lb * fold * (-n + TILT * e2), mid + Lb * (-0.5 * fold * n + 0.5 * e2)])


def _query(cross_pt, La, s, dq, n, swapped, fold=FOLD):
    q0 = cross_pt - s * La * dq
    q1 = q0 + La * dq
    side = np.cross(n, dq)
    mid = 0.5 * (q0 + q1)
    ends = [q1, q0] if swapped else [q0, q1]          # ascending vertex order: the detection sees D < 0 and swaps back
    return np.array(ends + [mid + La * fold * (n + TILT * side), mid + La * (0.5 * fold * n + 0.5 * side)])


def make_probe(center, La, Lb, sin, st, swapped, nx, kind, gap=0.5, phi=0.7, seed=0, axis=False):
    """the query edge over the target edge at gap * eps, the slot normal with n.x = nx, sin of the angle between the edges, closest points at (s, t) of the
    slot.  Each triangle's third vertex is folded away from the other edge (FOLD of its edge along -+n, a small TILT sideways) and each body has an apex
    off its triangle for the carrier tetrahedron.  axis: n = z, target along x, query along y.  Previous positions: the target moved rigidly, the query
    edge by another vector (0.2 eps_v dt sideways, a little along n): dx0 != gap n"""
    if axis:
        n, e1, e2 = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    else:
        n, e1, e2 = cn._frame(nx, phi + 0.37 * seed)
    s, t = st
    dq = np.sqrt(1 - sin * sin) * e1 + sin * e2 if sin < 1 else e2
    tgt = _target(center, Lb, t, n, e1, e2)
    qry = _query(center + gap * EPS * n, La, s, dq, n, swapped)
    rng = np.random.default_rng(2000 + seed)
    vt = 1e-5 * rng.normal(size=3)
    vq = vt + EH * (0.2 * np.cos(seed) * e1 + 0.2 * np.sin(seed) * e2) + 1e-6 * n
    return Probe(tgt, qry, tgt - vt, qry - vq, kind, gap < 1.0 and sin >= SIN_MIN and 0 < s < 1 and 0 < t < 1,
                 "La%g Lb%g sin%g st(%g,%g) %s nx%g kind%d" % (La, Lb, sin, s, t, "D<0" if swapped else "D>0", nx, kind), La, Lb, s, t, swapped)


class Scene:
    """probes on the lattice of contact_numpy; per kind of mu one target body and one query body (an unordered body pair is taken by its first descriptor
    only), four vertices per probe and body; faces: one triangle per probe and body; carriers: one tetrahedron (triangle, apex) per probe and body with
    mu = lam = 0; every vertex carries the border flag, so that the vertex-triangle projection of a query vertex, which lands on the target triangle's rim,
    lists nothing.  shared_target: every probe's query edge crosses the first probe's target edge"""
    def __init__(self, probes, shared_target=False, mass=cn.MASS, v_offset=0, body_offset=0):
        self.mass, self.mdt2 = mass, mass / DT ** 2
        probes = sorted(probes, key=lambda p: p.kind)
        self.probes, self.P = probes, len(probes)
        xs, ps, faces, bodies, pairs, tets = [], [], [], [], [], []
        self.tv, self.qv = np.zeros(self.P, int), np.zeros(self.P, int)      # first vertex of each probe's target / query quadruple
        nv = nf = 0
        for kind, mu in ((0, (MU_FIXED,)), (1, (None, CE_FACTOR)), (2, ("cloth_cloth",))):
            ids = [i for i, p in enumerate(probes) if p.kind == kind]
            if not ids:
                continue
            tids = ids[:1] if shared_target else ids
            v0, f0 = nv, nf
            for i in tids:
                self.tv[i] = nv
                xs.append(probes[i].tgt); ps.append(probes[i].ptgt)
                faces.append([nv, nv + 1, nv + 2]); tets.append([nv, nv + 1, nv + 2, nv + 3])
                nv += 4; nf += 1
            if shared_target:
                self.tv[ids] = v0
            bodies.append((v0, nv, f0, nf))
            v1, f1 = nv, nf
            for i in ids:
                self.qv[i] = nv
                xs.append(probes[i].qry); ps.append(probes[i].pqry)
                faces.append([nv, nv + 1, nv + 2]); tets.append([nv, nv + 1, nv + 2, nv + 3])
                nv += 4; nf += 1
            bodies.append((v1, nv, f1, nf))
            pairs.append((len(bodies) - 2, v1, nv) + mu)
        self.x, self.prev, self.nv = np.concatenate(xs), np.concatenate(ps), nv
        self.faces, self.tets, self.bodies, self.pairs = np.array(faces, np.int32), np.array(tets, np.int32), bodies, pairs
        self.border = np.ones(nv, np.int32)
        self.mu_of_kind = {0: MU_FIXED, 1: MU_CE * CE_FACTOR, 2: MU_CC}
        self.active = [i for i, p in enumerate(probes) if p.active]

    def cand(self, i):
        """global vertices (a0, a1, b0, b1) of probe i's candidate pair"""
        return [self.qv[i], self.qv[i] + 1, self.tv[i], self.tv[i] + 1]

    def slot_verts(self, i):
        q = self.qv[i]
        return [self.tv[i], self.tv[i] + 1] + ([q + 1, q] if self.probes[i].swapped else [q, q + 1])

    def idx(self):
        return np.array([self.slot_verts(i) for i in self.active], np.int32).reshape(-1, 4)

    def kinds(self):
        return np.array([self.probes[i].kind for i in self.active])


lattice = cn.lattice
SINS = (1.0, 0.3, SIN_MIN * (1 + 1e-6))
STS = ((0.45, 0.6), (1e-3, 1 - 1e-3), (1 - 1e-6, 1e-6))
LENS = ((LS[0], LS[0]), (LS[1], LS[1]), (LS[0], LS[1]), (LS[0], LS[0]), (LS[1], LS[1]))


def _cycle(i, c, **kw):
    """probe i of the crossed properties: edge lengths (1 / 150, 1e-4, and 1 / 150 over 1e-4), sin 1 / 0.3 / 1e-2 (1 + 1e-6), (s, t) mid-edge / (1e-3,
    1 - 1e-3) / (1 - 1e-6, 1e-6), D > 0 / D < 0, the four n.x, the three kinds"""
    La, Lb = LENS[i % 5]
    return make_probe(c, La, Lb, kw.pop("sin", SINS[(i + i // 3) % 3]), kw.pop("st", STS[(i // 2) % 3]), (i // 2 + i // 5) % 2 == 1, NX[(i + i // 8) % 4], i % 3, seed=i, **kw)


def geometry_probes(n=16):
    """the probes of the assembly tests + the four that the detection must leave out: sin = 1e-2 (1 - 1e-6), s = -1e-6, t = 1 + 1e-6, gap 1.5 eps"""
    cs = lattice(n + 4)
    out = [_cycle(i, cs[i]) for i in range(n)]
    out.append(make_probe(cs[n], LS[0], LS[0], SIN_MIN * (1 - 1e-6), STS[0], False, 0.1, 0, seed=50))
    out.append(make_probe(cs[n + 1], LS[0], LS[1], 1.0, (-1e-6, 0.6), False, 0.1, 1, seed=51))
    out.append(make_probe(cs[n + 2], LS[1], LS[0], 0.3, (0.45, 1 + 1e-6), True, -0.9, 2, seed=52))
    out.append(make_probe(cs[n + 3], LS[0], LS[0], 1.0, STS[0], False, 0.1, 0, gap=1.5, seed=53))
    return out


def launch_probes(nc, up=0.0):
    cs = [c + np.array([0.0, 0.0, up]) for c in lattice(nc)]
    return [_cycle(i, cs[i], gap=0.3 + 0.05 * (i % 9)) for i in range(nc)]


def reverse_probes(nc):
    """sin >= 0.3, both edge lengths, (s, t) mid-edge and near an end, D of both signs, the four n.x, the three kinds"""
    cs = lattice(nc)
    return [_cycle(i, cs[i], sin=(1.0, 0.3)[i % 2], st=STS[(i // 2) % 2], gap=0.3 + 0.05 * (i % 9)) for i in range(nc)]


def crowd_probes(n=70):
    """n query edges of 1e-3 m across ONE target edge of 5 cm: its two vertices have constraint rows of n entries"""
    c, Lb = np.zeros(3), 0.05
    n_, e1, e2 = cn._frame(0.1, 0.7)
    out = []
    for i in range(n):
        t = 0.3 + 0.4 * ((i * 7) % n) / n
        sin = (1.0, 0.6)[i % 2]
        dq = np.sqrt(1 - sin * sin) * e1 + sin * e2 if sin < 1 else e2
        s, La, gap = 0.3 + 0.01 * (i % 40), 1e-3, 0.3 + 0.005 * i
        tgt = _target(c, Lb, 0.5, n_, e1, e2, fold=0.1)     # (a shallow target and steep query triangles: no other edge pair comes within eps)
        qry = _query(tgt[0] + t * Lb * e1 + gap * EPS * n_, La, s, dq, n_, i % 3 == 1, fold=4.0)
        vq = EH * 0.1 * e1 * (1 + i % 4)
        out.append(Probe(tgt, qry, tgt, qry - vq, 0, True, "crowd %d" % i, La, Lb, s, t, i % 3 == 1))
    return out


def parallel_probes():
    """axis-aligned probes (target along x, query along y at the detection: sin = 1) for the state "exactly parallel": both lengths, D of both signs,
    the three kinds"""
    cs = lattice(6)
    return [make_probe(cs[i], LENS[i % 3][0], LENS[i % 3][1], 1.0, STS[0] if i < 3 else (0.3, 0.8), i % 2 == 1, 0.0, i % 3, seed=i, axis=True) for i in range(6)]


MASS_REVERSE = 2.0 ** 6     # m / dt^2 = 2^22 = 4.2e6: the power of two above the -3.3e6 that a penetrated probe of 1e-4 m at sin = 0.3 puts into the summed
#                            unprojected operator of the "rv" scenes (asserted on the CPU, tests/test_ee_elements_numpy.py); the read-back of p stays exact


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "geometry":
        return Scene(geometry_probes())
    if name == "crowd":
        return Scene(crowd_probes(), shared_target=True)
    if name == "parallel":
        return Scene(parallel_probes())
    if name.startswith("rv"):
        return Scene(reverse_probes(int(name[2:])), mass=MASS_REVERSE)
    assert name.startswith("nc")
    if name.endswith("up"):      # 0.06 m above the lattice: behind vertex-triangle probes of contact_numpy in one context (Merged)
        return Scene(launch_probes(int(name[2:-2]), up=0.06))
    return Scene(launch_probes(int(name[2:])))


class Merged:
    """vertex-triangle probes of contact_numpy (a contact_numpy.Scene) in front of edge-edge probes (a Scene built 0.06 m above them): one set of tables"""
    def __init__(self, vt, ee):
        self.vt, self.ee, self.mass, self.mdt2 = vt, ee, vt.mass, vt.mdt2
        o, nb, nf = vt.nv, len(vt.bodies), len(vt.faces)
        self.x, self.prev = np.concatenate([vt.x, ee.x]), np.concatenate([vt.prev, ee.prev])
        self.nv = len(self.x)
        self.faces, self.tets = np.concatenate([vt.faces, ee.faces + o]), np.concatenate([vt.tets, ee.tets + o])
        self.bodies = list(vt.bodies) + [(a + o, b + o, c + nf, d + nf) for a, b, c, d in ee.bodies]
        self.pairs = list(vt.pairs) + [(p[0] + nb, p[1] + o, p[2] + o) + tuple(p[3:]) for p in ee.pairs]
        self.border = np.concatenate([np.zeros(vt.nv, np.int32), ee.border])
        self.P = vt.P + ee.P

    def idx(self):
        return np.concatenate([self.vt.idx(), self.ee.idx() + self.vt.nv])


def probe_context(sc, frozen=None, max_n_constraints=None, ee=1):
    """engine context of a Scene or a Merged: contact_numpy.probe_context with the border flags and the key "contact_ee" """
    ctx = cn.probe_context(sc, frozen, max_n_constraints)
    ctx.set_border(sc.border)
    ctx.set_param("contact_ee", ee)
    return ctx


# ------------------------------------------------------------------------------------------------ what the construction must deliver, on the CPU
def vertex_triangle_sees_nothing(sc, x=None):
    """every vertex of a probe's query body projects onto the plane of the probe's target triangle outside the triangle (a barycentric weight below -0.01):
    its closest point lies on the rim, whose vertices carry the border flag"""
    x = sc.x if x is None else x
    for i in range(sc.P):
        tri = x[sc.tv[i]:sc.tv[i] + 3]
        for v in range(sc.qv[i], sc.qv[i] + 4):
            if not cn.barycentric(np.vstack([tri, x[v]])).min() < -0.01:
                return False
    return bool(sc.border.all())


def brute_force(sc, x=None):
    """ee_numpy.brute_force on the scene's tables: (idx, (s, t)) in list order"""
    return en.brute_force(sc.x if x is None else x, sc.faces, sc.bodies, [p[:3] for p in sc.pairs], EPS)


# ------------------------------------------------------------------------------------------------ records of a scene
def scene_records(xp, sc, dec=None, x=None, prev=None):
    """records of the qualifying probes in slot order (kind, probe: the descriptors in order, the query edges ascending)"""
    x, prev = sc.x if x is None else x, sc.prev if prev is None else prev
    out = []
    for i, p in enumerate(sc.probes):
        vs = sc.cand(i)
        d = [] if dec is not None else None
        rec = slot_records(xp, x[vs], prev[vs], sc.mu_of_kind[p.kind], SC, d)
        if dec is not None:
            dec.append((i, d))
        if rec is not None:
            rec["idx"] = [vs[o] for o in rec["order"]]
            rec["kind"], rec["probe"] = p.kind, i
            out.append(rec)
    return out


records_as_data, slot_rec = cn.records_as_data, cn.slot_rec
_fn, _bnd = cn._fn, cn._bnd


def check_records(sc, cons, R, offset=0):
    """the exported records against the restatement at the detection state: idx, mu exact, w[2] == 0 exactly, s, t, k, dx0, T, n within the bound (e64 over
    the state and eight one-ulp jitters of pos and prev: a rotation would change the branch of T), T orthogonal to n and its rows to each other within
    8 u; a slot whose s is that of the unswapped query edge is named"""
    with mp.workdps(50):
        rm = scene_records(MP, sc)
    with np.errstate(all="ignore"):
        copies = [scene_records(F64, sc)] + [scene_records(F64, sc, x=xj, prev=pj) for xj, pj in zip(jitters(sc.x, seed=1), jitters(sc.prev, seed=2))]
    assert len(cons["k"]) == len(rm) == len(sc.active), (len(cons["k"]), len(rm))
    assert all(len(c) == len(rm) for c in copies)
    assert np.array_equal(cons["idx"] - offset, sc.idx()) and np.array_equal(sc.idx(), np.array([r["idx"] for r in rm]))
    for s, r in enumerate(rm):
        i = r["probe"]
        assert cons["w"][s][2] == 0.0, s
        assert cons["mu"][s] == sc.mu_of_kind[sc.probes[i].kind], s
        for q, got, want in [("s", cons["w"][s][:1], r["w"][:1]), ("t", cons["w"][s][1:2], r["w"][1:2])] + [(q, cons[q][s], r[q]) for q in ("k", "dx0", "n", "T")]:
            hl = split(np.array(want, dtype=object).ravel())
            f = lambda c: c[s]["w"][:1] if q == "s" else c[s]["w"][1:2] if q == "t" else c[s][q]
            e64 = max(float(_fn(diff(np.array([float(v) for v in np.ravel(f(c))]), hl))) for c in copies)
            err, bnd = float(_fn(diff(np.ravel(got), hl))), float(_bnd(e64, _fn(hl[0])))
            if q == "s" and err > bnd and abs(float(got[0]) - (1 - hl[0][0])) <= bnd:
                raise AssertionError("slot %d: s is that of the unswapped query edge (s -> 1 - s left out of the swap)" % s)
            ratio(R, "record " + q, err, bnd)
        n, t1, t2 = cons["n"][s], cons["T"][s][:3], cons["T"][s][3:]
        assert max(abs(n @ t1), abs(n @ t2), abs(t1 @ t2)) <= 8 * U, (s, "T not orthogonal")


# ------------------------------------------------------------------------------------------------ evaluation states
def _geom(sc, recs):
    out = []
    for r in recs:
        vs = r["idx"]
        f = lambda v: np.array([float(t) for t in v])
        out.append(dict(vs=vs, n=f(r["n"]), T=f(r["T"]).reshape(2, 3), s=float(r["w"][0]), t=float(r["w"][1]), dx0=f(r["dx0"]), i=r["probe"],
                        La=sc.probes[r["probe"]].La, Lb=sc.probes[r["probe"]].Lb))
        out[-1]["s2"] = float(out[-1]["T"][0] @ out[-1]["T"][0])
    return out


def _dx(x, g):
    v = g["vs"]
    return (x[v[2]] * (1 - g["s"]) + x[v[3]] * g["s"]) - (x[v[0]] * (1 - g["t"]) + x[v[1]] * g["t"]) - g["dx0"]


def _move_q(x, g, delta):
    x[g["vs"][2]] = x[g["vs"][2]] + delta
    x[g["vs"][3]] = x[g["vs"][3]] + delta


def _set_d(sc, x, geo, dfac):
    """the query edge moved along n until the line distance is dfac eps"""
    for g in geo:
        _move_q(x, g, (dfac * EPS - float(en.line_distance(x[g["vs"]]))) * g["n"])
    return x


def _slip(sc, geo, rfac, direction, dfac=0.5, r_abs=None, x=None):
    """the query edge moved in the tangent plane until u = r (cos, sin)(direction): r = rfac eps_v dt (or r_abs), then along n to d = dfac eps"""
    x = sc.x.copy() if x is None else x
    for k, g in enumerate(geo):
        r = EH * rfac if r_abs is None else r_abs
        ang = {"t1": 0.0, "t2": np.pi / 2, "oblique": 0.4 + 0.9 * k}[direction]
        for _ in range(2):       # (the second pass takes out the rounding of the first where r is far below the first move)
            _move_q(x, g, (np.array([r * np.cos(ang), r * np.sin(ang)]) - g["T"] @ _dx(x, g)) @ g["T"] / g["s2"])
    return _set_d(sc, x, geo, dfac)


def _turn(sc, geo, sin, x=None):
    """the query edge turned about the common normal through its closest point until sin(angle between the edges) = sin; d stays where it was"""
    x = sc.x.copy() if x is None else x
    for g in geo:
        v = g["vs"]
        e1 = (x[v[1]] - x[v[0]]) / np.linalg.norm(x[v[1]] - x[v[0]])
        e2 = np.cross(g["n"], e1)
        qs = x[v[2]] * (1 - g["s"]) + x[v[3]] * g["s"]
        dq = np.sqrt(1 - sin * sin) * e1 + sin * e2
        x[v[2]], x[v[3]] = qs - g["s"] * g["La"] * dq, qs + (1 - g["s"]) * g["La"] * dq
    return x


def _slide_off(sc, geo):
    """both edges moved along themselves: the closest points of the current lines lie at s = -0.2 - ... and t = 1.3 + ..., outside both edges; the records kept"""
    x = sc.x.copy()
    for g in geo:
        v = g["vs"]
        x[v[2:]] = x[v[2:]] + 1.2 * (x[v[3]] - x[v[2]])
        x[v[:2]] = x[v[:2]] - 1.3 * (x[v[1]] - x[v[0]])
    return x


def _bump(sc, geo):
    x = sc.x.copy()
    rng = np.random.default_rng(12)
    for g in geo:
        for k, v in enumerate(g["vs"]):
            x[v] = x[v] + 0.05 * (g["Lb"] if k < 2 else g["La"]) * rng.uniform(-1, 1, 3)
    return x


def _parallel(sc, geo):
    """axis-aligned probes: the query edge laid along x over the target edge, y and z of its two vertices the same bits: a x b == 0.0"""
    x = sc.x.copy()
    for g in geo:
        v = g["vs"]
        qs = x[v[2]] * (1 - g["s"]) + x[v[3]] * g["s"]
        x[v[2]] = np.array([qs[0] - g["s"] * g["La"], qs[1], qs[2]])
        x[v[3]] = np.array([qs[0] + (1 - g["s"]) * g["La"], qs[1], qs[2]])
    return x


def _reverse_mix(sc, geo):
    """x_2 of the reverse-step tests (records lagged at x_1 = the scene's positions, previous positions = positions): slot k sticks (0.3 eps_v dt, k % 4 == 0),
    slips (10 eps_v dt, 1), keeps its four vertices (2), is penetrated to -0.5 eps with 0.3 eps_v dt (3)"""
    x = sc.x.copy()
    for k, g in enumerate(geo):
        if k % 4 == 2:
            continue
        r, d = [(0.3 * EH, 0.5), (10 * EH, 0.5), None, (0.3 * EH, -0.5)][k % 4]
        ang = 0.4 + 0.9 * k
        for _ in range(2):
            _move_q(x, g, (np.array([r * np.cos(ang), r * np.sin(ang)]) - g["T"] @ _dx(x, g)) @ g["T"] / g["s2"])
        _move_q(x, g, (d * EPS - float(en.line_distance(x[g["vs"]]))) * g["n"])
    return x


STATES = {
    "rest": lambda sc, geo: sc.x.copy(),
    "d=eps(1-1e-6)": lambda sc, geo: _set_d(sc, sc.x.copy(), geo, 1 - 1e-6),
    "d=eps(1+1e-6)": lambda sc, geo: _set_d(sc, sc.x.copy(), geo, 1 + 1e-6),
    "d=0.5eps": lambda sc, geo: _set_d(sc, sc.x.copy(), geo, 0.5),
    "d=-0.5eps": lambda sc, geo: _set_d(sc, sc.x.copy(), geo, -0.5),
    "d=-3eps": lambda sc, geo: _set_d(sc, sc.x.copy(), geo, -3.0),
    "d=2eps": lambda sc, geo: _set_d(sc, sc.x.copy(), geo, 2.0),
    "r=1e-9(1-1e-3)": lambda sc, geo: _slip(sc, geo, None, "oblique", r_abs=R_GUARD * (1 - 1e-3)),
    "r=1e-9(1+1e-3)": lambda sc, geo: _slip(sc, geo, None, "oblique", r_abs=R_GUARD * (1 + 1e-3)),
    "r=eh(1-1e-6)": lambda sc, geo: _slip(sc, geo, 1 - 1e-6, "oblique"),
    "r=eh(1+1e-6)": lambda sc, geo: _slip(sc, geo, 1 + 1e-6, "oblique"),
    "r=0.3eh t1": lambda sc, geo: _slip(sc, geo, 0.3, "t1"),
    "r=0.3eh oblique": lambda sc, geo: _slip(sc, geo, 0.3, "oblique"),
    "r=10eh t2": lambda sc, geo: _slip(sc, geo, 10.0, "t2"),
    "r=10eh oblique, d=2eps": lambda sc, geo: _slip(sc, geo, 10.0, "oblique", dfac=2.0),
    "r=1e3eh t1": lambda sc, geo: _slip(sc, geo, 1e3, "t1"),
    "r=1e3eh oblique, d=-0.5eps": lambda sc, geo: _slip(sc, geo, 1e3, "oblique", dfac=-0.5),
    "turned to sin=1e-2": lambda sc, geo: _turn(sc, geo, 1e-2),
    "turned to sin=1e-3": lambda sc, geo: _turn(sc, geo, 1e-3),
    "turned to sin=1e-5": lambda sc, geo: _turn(sc, geo, 1e-5),
    "slid off the ends": _slide_off,
    "bump": _bump,
    "exactly parallel": _parallel,
    "reverse mix": _reverse_mix,
}
SPECIAL = ("exactly parallel", "reverse mix")     # states of their own scenes ("parallel"; "rv*" with prev == pos at the detection)
ASSEMBLY_STATES = [k for k in STATES if k not in SPECIAL]


@functools.lru_cache(maxsize=None)
def own_records(name, lagged=True):
    sc = scene(name)
    return scene_records(F64, sc, prev=None if lagged else sc.x)


def state_positions(name, state, lagged=True):
    sc = scene(name)
    return STATES[state](sc, _geom(sc, own_records(name, lagged)))


def parallel_jitters(X, n=8, seed=0):
    """one-ulp jitters of a slot's positions that stay inside the construction of the exactly parallel state: every coordinate moves by one ulp, and the two
    vertices of an edge get the same y and the same z again, so that a x b stays zero bit for bit"""
    out = jitters(X, n=n, seed=seed)
    for J in out:
        J[1, 1:], J[3, 1:] = J[0, 1:], J[2, 1:]
    return out


def jitter_of(state):
    return parallel_jitters if state == "exactly parallel" else jitters


def expected(cons, pos, spd, frozen=None, z=None, state=None):
    return cn.Expected(cons, pos, spd, frozen, z, model=EE, jitter=jitter_of(state))


# ------------------------------------------------------------------------------------------------ the float64 restatement in the kernels' place
def f64_records(name, lagged=True):
    return records_as_data(own_records(name, lagged))


def f64_kernels(name, pos, spd, frozen=None, rot=1, lagged=True, cons=None):
    """what the engine returns, by the float64 restatement evaluated in a rotated frame: blocks, masked blocks, gradient, dense contact operator, energy"""
    sc = scene(name)
    cons = f64_records(name, lagged) if cons is None else cons
    nv = sc.nv
    fz = np.zeros(3 * nv, bool) if frozen is None else np.asarray(frozen, bool)
    R = rotations()[rot]
    blocks, masked, g, op, E = [], [], np.zeros((nv, 3)), np.zeros((nv, 3, nv, 3)), 0.0
    for s in range(len(cons["k"])):
        vs = cons["idx"][s]
        rec = slot_rec(cons, s)
        with np.errstate(all="ignore"):
            a = cn._back(cn._arr(slot_eval(F64, pos[vs] @ R.T, cn._rot_rec(rec, R), SC, spd)), R)
        f12 = fz[cn.dofs(vs)]
        B = a["H"].reshape(12, 12)
        Mk = np.where(np.outer(~f12, ~f12), B, 0.0)
        blocks.append(B); masked.append(Mk)
        E += float(a["E"])
        for i in range(4):
            g[vs[i]] += a["g"][i] * ~f12[3 * i:3 * i + 3]
            for j in range(4):
                op[vs[i], :, vs[j], :] += Mk.reshape(4, 3, 4, 3)[i, :, j, :]
    return cons, dict(blocks=np.array(blocks), masked=np.array(masked), g=g, op=op.reshape(3 * nv, 3 * nv), E=E)


def f64_reverse(name, pos, z, cons, frozen=None):
    """(sum per vertex of the float64 backprop entries, tmp_z_frozen's contact part) in slot order"""
    sc = scene(name)
    fz = np.zeros(3 * sc.nv, bool) if frozen is None else np.asarray(frozen, bool)
    z = np.asarray(z, float).reshape(-1, 3)
    acc, zf = np.zeros((sc.nv, 3)), np.zeros(3 * sc.nv)
    for s in range(len(cons["k"])):
        vs, rec = cons["idx"][s], slot_rec(cons, s)
        acc[vs] += np.array(slot_reverse(F64, pos[vs], rec, z[vs].ravel())["acc"]).reshape(4, 3)
        H = np.array(slot_eval(F64, pos[vs], rec)["H"], float)
        d12 = cn.dofs(vs)
        f12 = fz[d12]
        zs = np.where(f12, 0.0, z[vs].ravel())
        zf[d12[f12]] -= (H[:, f12].T @ zs)
    return acc, zf.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ decisions
def detection_decisions(xp, sc, x=None, prev=None):
    d = []
    with mp.workdps(50):
        scene_records(xp, sc, dec=d, x=x, prev=prev)
    return [("det", i, n, v) for i, dd in d for n, v in dd]


def eval_decisions(xp, X, rec):
    dd = []
    with mp.workdps(50):
        slot_eval(xp, X, rec, SC, 0, dd)
    return dd


def _same(a, b, tag):
    assert [p[:-1] for p in a] == [q[:-1] for q in b], tag
    for p, q in zip(a, b):
        da, db = float(p[-1]), float(q[-1])
        assert abs(da) >= SAFE and abs(db) >= SAFE and (da > 0) == (db > 0), (tag, p, q)


def decisions_safe(name, state, lagged=True):
    """every decision of the detection (mp, float64, the eight jittered copies of pos and prev that the records' e64 is taken from) and of the evaluation
    (mp, float64, the six rotated and eight jittered copies that e64 is taken from) has the same outcome at least SAFE from its threshold.  The exception:
    the state "exactly parallel", whose construction fixes a x b == 0.0: asserted bit for bit on the float64 evaluation of the state and of its rotations
    (signed permutations keep the edges on an axis) and of its jittered copies, which move every coordinate by one ulp and keep the y and the z of an
    edge's two vertices the same bits (parallel_jitters: free jitters would leave the construction)"""
    sc = scene(name)
    prev = None if lagged else sc.x
    dm = detection_decisions(MP, sc, prev=prev)
    _same(dm, detection_decisions(F64, sc, prev=prev), (name, "detection"))
    for xj, pj in zip(jitters(sc.x, seed=1), jitters(sc.prev if lagged else sc.x, seed=2)):
        _same(dm, detection_decisions(F64, sc, x=xj, prev=pj if lagged else xj), (name, "detection, jittered"))
    cons = f64_records(name, lagged)
    pos = state_positions(name, state, lagged)
    for s in range(len(cons["k"])):
        X, rec = pos[cons["idx"][s]], slot_rec(cons, s)
        mine = eval_decisions(MP, X, rec)
        copies = [(X @ R.T, cn._rot_rec(rec, R)) for R in rotations()]
        if state == "exactly parallel":
            for Xc, _ in copies + [(Xj, rec) for Xj in parallel_jitters(X, seed=int(abs(X).sum() * 1e9) % 1000)]:
                a, b = Xc[1] - Xc[0], Xc[3] - Xc[2]
                assert not np.cross(a, b).any() and not np.array(_cross(list(a), list(b))).any(), (name, s, "a x b is not zero bit for bit")
            assert [n for n, _ in mine] == ["r_eh", "r_guard"], (name, s, "the normal part records no decision where C == 0")
        copies += [(Xj, rec) for Xj in jitter_of(state)(X, n=8, seed=int(abs(X).sum() * 1e9) % 1000)]
        for Xc, rc in copies:
            with np.errstate(all="ignore"):
                _same([(s,) + t for t in mine], [(s,) + t for t in eval_decisions(F64, Xc, rc)], (name, state, s))
    return True
