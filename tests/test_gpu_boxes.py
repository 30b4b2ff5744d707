"""Rounded-box colliders (tsl_set_boxes; csrc/k_box.hpp) through the C ABI.  The reference has no such term: it is checked against
the dense NumPy restatement (tests/box_numpy.py), the capsule kernels where the half extents are (L/2, 0, 0), the sphere kernels where they are
(0, 0, 0), and whole-rollout differences.  The idiom is that of tests/test_gpu_capsules.py: a box quantity of a state is the difference against
the same state with k_box = 0 -- no box kernel runs there, and the rest is formed by the same launches in both -- and K = 2e5 N/m, the size of
the cloth's own diagonal entries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_numpy as bn  # noqa: E402
import capsule_numpy as kn  # noqa: E402
import collider_numpy as cn  # noqa: E402
import handle_numpy as hn  # noqa: E402
import sphere_numpy as sn  # noqa: E402
import tie_numpy as tn  # noqa: E402
from thinshelllab_amd._lib import EXPORTS  # noqa: E402

assert "tsl_set_boxes" in EXPORTS   # (without the feature the module does not import)

pytestmark = pytest.mark.gpu

K = 2.0e5
DX = 0.1 / 15
RAD = np.array([0.01, 0.01])
MU = np.array([0.5, 0.3])
QID = np.array([1.0, 0.0, 0.0, 0.0])


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


class _State:
    """one state of a context: positions, start-of-step positions, zero velocity, rest angles; energy / gradient / operator of it as NumPy"""

    def __init__(self, ctx, x, xp, ref):
        self.ctx = ctx
        self.pos = _dev(x); self.prev = _dev(xp); self.vel = torch.zeros_like(self.pos)
        self.ref = ref

    def energy(self):
        return self.ctx.energy(self.pos, self.prev, self.vel, self.ref)

    def grad(self, spd=0):
        F = torch.zeros(self.pos.numel(), dtype=torch.float64, device="cuda")
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd, grad=F)
        return F.cpu().numpy().reshape(-1, 3)

    def operator(self, spd):
        """the full operator, dense: the static matrix plus the masked blocks of every constraint slot"""
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd)
        A = self.ctx.matrix_csr().toarray()
        if len(self.ctx.constraints()["idx"]):
            idx, blk = self.ctx.constraints()["idx"], self.ctx.contact_blocks(True)
            for c in range(len(blk)):
                d = np.concatenate([3 * v + np.arange(3) for v in idx[c]])
                A[np.ix_(d, d)] += blk[c]
        return A

    def part(self, fun, k=K, with_base=False, key="k_box"):
        """fun() with k_box = k minus fun() with k_box = 0 (with_base: and the latter)"""
        self.ctx.set_param(key, k)
        a = fun()
        self.ctx.set_param(key, 0.0)
        b = fun()
        self.ctx.set_param(key, k)
        return (a - b, b) if with_base else a - b


def _drape(N, pin=True, perturb=0.0, newton_cap=200):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=DX * N, N=N, M=N, pin_row=pin, perturb=perturb, newton_cap=newton_cap)
    s.init_all()
    return s


def _quat(theta, q=QID):
    from thinshelllab_amd.engine import frames
    return frames.quat_normalize(frames.quat_mul(frames.quat_exp(theta), q))


def _gap_draw(rng, eps):
    """a gap on either side of the shell, at least a quarter of it away from it: in (-0.5, 0.75) eps or in (1.25, 2.5) eps"""
    g = rng.uniform(-0.5, 2.0)
    return (g if g < 0.75 else g + 0.5) * eps


def pushed(x0, sel, n_side, eps, eh, seed):
    """The vertices `sel` of a flat horizontal sheet (n_side cells of DX along x) pushed partly through two rounded boxes (r = 10 mm) under it whose
    rounded tops lie in the sheet, both of them translating and turning by about eps_v dt over the step.  Box 0 is level and square under the middle,
    half as wide as the sheet plus 0.008 DX: the vertex rows and columns a quarter of the sheet from the middle lie 0.004 DX inside its edge lines,
    the ones beyond them over its edges and, on the diagonals, over its corners.  Only the vertices up to one spacing beyond the core box are pushed
    against box 0 (the others keep their place and are masked out for it: a vertex far beyond an edge of a box of this radius would have to travel
    centimetres).  Distances and start-of-step distances to box 0 on either side of the shell independently, slips relative to the box's material
    point of 0, 0.3 and 3 times eps_v dt (the last carries vertices of those columns from the face over the edge line: free differs from free0); box 1,
    a yawed bar a third of the sheet beside, its top half a shell higher, meets whatever heights that gives, on the vertices up to 0.35 of the sheet's
    width from its centre.  Every length is below 0.1 m, and the gaps of box 0 keep a quarter of the shell away from it.
    (centres, quats, previous centres, previous quats, half extents, x_prev, x, the vertices pushed against box 0, the vertices that see box 1)"""
    rng = np.random.default_rng(seed)
    x, xp = x0.copy(), x0.copy()
    mid = x0[sel].mean(axis=0)
    w = n_side * DX
    hq = (n_side // 4 + 0.004) * DX
    h = np.array([[hq, hq, 0.01], [0.15 * w, 0.3 * w, 0.008]])
    c = np.array([[mid[0], mid[1], mid[2] - RAD[0] - h[0, 2]], [mid[0] + w / 3, mid[1], mid[2] - RAD[1] - h[1, 2] + 0.5 * eps]])
    q = np.array([QID, _quat([0.0, 0.0, 0.4])])
    cp = c - np.array([[0.4 * eh, 0.2 * eh, 0.6 * eh], [-0.2 * eh, 0.4 * eh, 0.2 * eh]])
    turn = np.array([[0.6, -0.8, 1.0], [-0.5, 0.7, 0.9]]) * (eh / hq)   # (a point at the edge of box 0 moves by about eps_v dt)
    qp = np.array([_quat(-turn[j], q[j]) for j in range(2)])
    R, R0 = np.array([bn.quat_to_R(a) for a in q]), np.array([bn.quat_to_R(a) for a in qp])
    near = [int(v) for v in sel if np.abs(x0[v, :2] - mid[:2]).max() < hq + 1.01 * DX]
    quarter = (n_side // 4) * DX
    # two vertices of each of the two columns a quarter from the middle: inside both shells, 3 eps_v dt of slip along x and outwards -- an axis is
    # clamped at x while it is free at x_prev; the four vertices on the diagonals beyond the corners: inside both shells
    col = {}
    for side, ang in ((-1.0, np.pi), (1.0, 0.0)):
        for v in [u for u in near if abs(x0[u, 0] - (mid[0] + side * quarter)) < 1e-6 * DX and abs(x0[u, 1] - mid[1]) < quarter - 0.5 * DX][1:3]:
            col[v] = (3.0 * eh, ang)
    for v in near:
        if (np.abs(x0[v, :2] - mid[:2]) > hq).all():
            col[v] = (rng.choice([0.3 * eh, 3.0 * eh]), rng.uniform(0, 2 * np.pi))
    for v in near:
        P0 = bn.Pair(x0[v], x0[v], cp[0], R0[0], cp[0], R0[0], h[0], RAD[0], 0.0, 1.0, 1.0, 1.0)
        n0, b0 = P0.n, P0.b
        g0, slip, ang, want = _gap_draw(rng, eps), rng.choice([0.0, 0.3 * eh, 3.0 * eh]), rng.uniform(0, 2 * np.pi), _gap_draw(rng, eps)
        if v in col:
            g0, (slip, ang), want = 0.3 * eps, col[v], 0.2 * eps
        xp[v] = cp[0] + R0[0] @ b0 + (RAD[0] + g0) * n0
        t = np.array([np.cos(ang), np.sin(ang), 0.0]); t -= n0 * (n0 @ t); t /= np.linalg.norm(t)
        base = xp[v] + ((c[0] + R[0] @ b0) - (cp[0] + R0[0] @ b0)) + slip * t
        al = 0.0
        for _ in range(12):   # (the gap grows with the shift along n0 at the rate n . n0, which is one but for a vertex that crossed an edge line)
            P = bn.Pair(base + al * n0, xp[v], c[0], R[0], cp[0], R0[0], h[0], RAD[0], 0.0, 1.0, 1.0, 1.0)
            al += (want - P.d) / max(float(P.n @ n0), 0.5)
        x[v] = base + al * n0
    near1 = [int(v) for v in sel if np.linalg.norm(x0[v, :2] - c[1, :2]) < 0.35 * w]
    return c, q, cp, qp, h, xp, x, np.array(near), np.array(near1)


def _table(c, q, cp, qp, h, mask, eps, eh, rad=RAD, mu=MU, k=K):
    """the arguments of the restatement behind (x, xp)"""
    return (c, np.array([bn.quat_to_R(a) for a in q]), cp, np.array([bn.quat_to_R(a) for a in qp]), h, rad, mu, mask, k, eps, eh)


def branches(x, xp, A):
    """asserts that the state walks through every branch; returns the active set"""
    c, R, cp, R0, h, r, mu, mask, k, eps, eh = A
    act, act0, reg, reg0 = bn.active_sets(x, xp, *A)
    on = reg != 9
    rw = np.zeros(act.shape)
    for v, j, P in bn.pairs(x, xp, *A):
        rw[v, j] = P.r_w
    fr = act0 & (mu[None, :] > 0)
    for ia in (True, False):
        for ib in (True, False):
            assert (on & (act == ia) & (act0 == ib)).any()
    assert (fr & (rw < 1e-9)).any() and (fr & (rw > 1e-9) & (rw < eh)).any() and (fr & (rw > eh)).any()
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any() and (mask == 0).any() and (on.sum(axis=1) == 1).any()
    both = act[:, 0] & fr[:, 0]
    for region in (2, 1, 0):     # the face, the edges and the corners of box 0 carry normal force and friction
        assert (both & (reg[:, 0] == region)).any() and (both & (reg0[:, 0] == region)).any(), region
    change = both & (reg[:, 0] != reg0[:, 0])
    print("pairs of box 0 with normal force and friction: %d, of them over face / edge / corner %s, with an axis clamped at x and free at x_prev %d, the other way round %d"
          % (both.sum(), [int((both & (reg[:, 0] == q)).sum()) for q in (2, 1, 0)], (change & (reg0[:, 0] > reg[:, 0])).sum(), (change & (reg0[:, 0] < reg[:, 0])).sum()))
    assert (change & (reg0[:, 0] == 2) & (reg[:, 0] == 1)).any()
    for j in range(len(r)):
        assert np.abs(c[j] - cp[j]).min() > 0 and np.abs(R[j] - R0[j]).max() > 0.1 * eh / 0.1
    # the premise of the 1e-12 bound: the rounding of x - c against the smallest |d - eps| of an active pair
    arm = max(np.linalg.norm(P.x - P.c) for v, j, P in bn.pairs(x, xp, *A))
    gaps = [min([min(abs(P.d - eps) if P.act else 1.0, abs(P.d0 - eps) if P.act0 else 1.0) for v, j, P in bn.pairs(x, xp, *A) if j == jj]) for jj in range(len(r))]
    print("largest |x - c| %.3e m, smallest |d - eps| of an active pair of box 0 %.3e m (of any box %.3e m): e64 |x - c| / |d - eps| = %.2e"
          % (arm, gaps[0], min(gaps), 2.2e-16 * arm / gaps[0]))
    assert arm <= 0.1 and 2.2e-16 * arm / gaps[0] < 1e-12
    return act


def _frozen_pattern(fz0, touched):
    """on top of the scene's own frozen dofs: all dofs of one touched vertex, one dof of a second, two of a third"""
    fz = fz0.copy()
    v0, v1, v2 = touched[:3]
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


FORCE_GROUPS = ((0, 3), (3, 6))
GRAD_GROUPS = ((0, 3), (3, 6), (6, 9), (9, 12), (12, 13), (13, 14))


def _check_state(S, x, xp, A, fz_list):
    """energy, gradient, operator in the spd modes 0, 1, 2 and with spd_literal, and the read-outs, of one state against the restatement.  Bound: 1e-12
    of the largest box entry (of each column group for the read-outs), the rods' and the spheres' bound."""
    ctx = S.ctx
    NV = len(x)
    assert ctx.box_count() == len(A[0])
    e_np, g_np = bn.energy(x, xp, *A), bn.gradient(x, xp, *A)
    H_ex, H_pr = bn.hessian(x, xp, *A, exact=True), bn.hessian(x, xp, *A, exact=False)
    B_np = bn.blocks(x, xp, *A)
    inside = np.zeros((3 * NV, 3 * NV), bool)
    for v in np.nonzero(np.abs(B_np).max(axis=(1, 2)) > 0)[0]:
        inside[3 * v:3 * v + 3, 3 * v:3 * v + 3] = True
    assert np.abs(H_ex - H_pr).max() > 1e-9 * np.abs(H_ex).max()          # (the curvature term is a thousand times over the bound)
    for frozen in fz_list:
        ctx.set_frozen(frozen.reshape(-1))
        fzb = frozen.astype(bool)
        free = (~fzb).ravel()
        e = S.part(S.energy)
        print("energy %.17g restatement %.17g rel %.2e" % (e, e_np, abs(e - e_np) / abs(e_np)))
        assert abs(e - e_np) <= 1e-12 * abs(e_np)
        g = S.part(S.grad)
        gm = g_np * ~fzb
        print("gradient err / max %.2e" % (np.abs(g - gm).max() / np.abs(gm).max()))
        assert np.abs(g - gm).max() <= 1e-12 * np.abs(gm).max() and (g[fzb] == 0).all()
        ff = np.outer(free, free)
        big = np.abs(H_ex * ff).max()
        got = {}
        for tag, spd, lit in (("spd 0", 0, 0), ("spd 1", 1, 0), ("spd 2", 2, 0), ("literal", 1, 1)):
            ctx.set_param("spd_literal", lit)
            D, Ab = S.part(lambda spd=spd: S.operator(spd), with_base=True)
            ctx.set_param("spd_literal", 0)
            Hm = (H_ex if spd == 0 else H_pr) * ff
            print("%s: operator err / largest box entry %.2e, asymmetric entries of the difference / of the rest %d / %d"
                  % (tag, np.abs(D - Hm).max() / big, (D != D.T).sum(), (Ab != Ab.T).sum()))
            assert np.abs(D - Hm).max() <= 1e-12 * big
            assert (D[~inside] == 0).all() and (D[~free] == 0).all() and (D[:, ~free] == 0).all()
            assert not ((D != D.T) & (Ab == Ab.T)).any()
            got[tag] = (D, Ab)
        # spd 0 against spd 1: exactly the curvature term, which has lost the free axes of a face or an edge
        curv = H_ex - H_pr
        cb = bn.curvature_blocks(x, xp, *A)
        for v in range(NV):
            assert np.abs(curv[3 * v:3 * v + 3, 3 * v:3 * v + 3] - cb[v]).max() <= 1e-12 * big
        dc = (got["spd 0"][0] - got["spd 1"][0]) - curv * ff
        print("spd 0 - spd 1 against the curvature term: %.2e of the largest box entry (the term itself %.2e)" % (np.abs(dc).max() / big, np.abs(curv * ff).max() / big))
        assert np.abs(dc).max() <= 1e-12 * big
        for tag in ("spd 2", "literal"):   # the projected modes add the same numbers: the same bits wherever the rest of the operator has the same bits
            D1, A1 = got["spd 1"]; D2, A2 = got[tag]
            same = (A1 == A2) & inside
            assert (D1[same] == D2[same]).all() and np.abs(D1 - D2).max() <= 1e-12 * big
        # the read-outs (frozen dofs: not masked in the force, not counted in the gradients)
        fo, fo_np = ctx.box_force(S.pos, S.prev), bn.force(x, xp, *A)
        pn = np.random.default_rng(11).normal(size=(NV, 3))
        bg, bg_np = ctx.box_grad(S.pos, S.prev, _dev(pn.reshape(-1))), bn.box_grad(x, xp, pn, frozen, *A)
        assert fo.shape == fo_np.shape == (len(A[0]), 6) and bg.shape == bg_np.shape == (len(A[0]), 14)
        for lo, hi in FORCE_GROUPS:
            print("  box_force[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(fo - fo_np)[:, lo:hi].max() / np.abs(fo_np[:, lo:hi]).max()))
            assert np.abs(fo - fo_np)[:, lo:hi].max() <= 1e-12 * np.abs(fo_np[:, lo:hi]).max()
        for lo, hi in GRAD_GROUPS:
            print("  box_grad[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(bg - bg_np)[:, lo:hi].max() / np.abs(bg_np[:, lo:hi]).max()))
            assert np.abs(bg - bg_np)[:, lo:hi].max() <= 1e-12 * np.abs(bg_np[:, lo:hi]).max()
        assert np.abs(bg_np).min() > 0 and np.abs(fo_np).min() > 0


def _masks(NV, near, near1):
    """partial masks: box 0 on the vertices pushed against it, box 1 on those about it; then vertices without any box, with one box only"""
    mask = np.zeros(NV, np.uint8)
    mask[near1] = 2
    mask[near] |= 1
    n = list(near)
    mask[[n[3], n[len(n) // 2]]] = 0
    mask[[n[5], n[len(n) // 2 + 1]]] &= 2
    mask[[n[7], n[-4]]] &= 1
    return mask


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("N", [8, 20])
def test_bare_cloth_matches_the_restatement(N):
    """N = 8: the 9 x 9-vertex cloth on the single-stream path, two waves; N = 20: 441 vertices, two workgroups with a partial one"""
    s = _drape(N)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    NV = s.tot_NV
    assert NV == (N + 1) ** 2 and ctx.contact_counts() == (0, 0)
    c, q, cp, qp, h, xp, x, near, near1 = pushed(s.pos.to_numpy(), np.arange(NV), N, eps, eh, seed=N)
    mask = _masks(NV, near, near1)
    A = _table(c, q, cp, qp, h, mask, eps, eh)
    act = branches(x, xp, A)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    assert fz0.any()
    ctx.set_boxes(c, q, h, RAD, MU, mask)
    ctx.set_box_poses(c, q, cp, qp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, x, xp, A, [fz0, _frozen_pattern(fz0, touched)])
    # new poses alone: the table follows; without previous poses the boxes are at rest
    ctx.set_frozen(fz0.reshape(-1))
    c2 = c + [[1e-4, 0.0, -2e-4], [0.0, 1e-4, 1e-4]]
    q2 = np.array([_quat([2e-3, -1e-3, 3e-3], q[0]), _quat([-1e-3, 2e-3, 1e-3], q[1])])
    e_old = bn.energy(x, xp, *A)
    for pc, pq, rc, rq in ((cp, qp, cp, qp), (None, None, c2, q2)):
        ctx.set_box_poses(c2, q2, pc, pq)
        e = S.part(S.energy)
        e_np = bn.energy(x, xp, *_table(c2, q2, rc, rq, h, mask, eps, eh))
        assert abs(e - e_np) <= 1e-12 * abs(e_np) and abs(e_np - e_old) > 1e-3 * abs(e_np)
    s._close_ctx()


def test_cloth_with_bodies_matches_the_restatement():
    """Scene_balancing with a 9 x 9-vertex cloth: bodies and contact pairs, so the assembly takes the three-stream schedule (assemble_enqueue_early)"""
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=DX * 8, cloth_N=8, cloth_M=8)
    s.init_all()
    ctx = s._ensure_ctx()
    ctx.set_param("tet_warm", 0)   # (two assemblies of one state differ in the last bits of the bodies' blocks otherwise; the differences ask for exact zeros)
    ctx.set_param("contact", 0)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    cl = s.cloths[0]
    assert cl.NV == 81 and ctx.n_body > 1
    NV = s.tot_NV
    cloth = np.arange(cl.offset, cl.offset + cl.NV)
    c, q, cp, qp, h, xp, x, near, near1 = pushed(s.pos.to_numpy(), cloth, 8, eps, eh, seed=5)
    mask = _masks(NV, near, near1)          # (the bodies see no box)
    A = _table(c, q, cp, qp, h, mask, eps, eh)
    act = branches(x, xp, A)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_boxes(c, q, h, RAD, MU, mask)
    ctx.set_box_poses(c, q, cp, qp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, x, xp, A, [fz0, _frozen_pattern(fz0, touched)])
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ the two limits, kernel against kernel
def _limit_state(s, rng, L):
    """a box that moves and turns under the middle of the sheet, its first axis along x; the vertices of the three middle rows about it: gaps on either
    side of the shell, slips of 0, 0.3 and 3 eps_v dt.  L = 0: about its centre only."""
    eps, eh = s.eps_contact, s.eps_v * s.dt
    x0 = s.pos.to_numpy()
    mid = x0.mean(axis=0)
    rad = 0.01
    c = np.array([[mid[0], mid[1], mid[2] - rad]])
    q = _quat([0.0, 0.02, 0.05])[None]
    cp = c - [[0.4 * eh, 0.2 * eh, 0.6 * eh]]
    qp = _quat([4e-3, -6e-3, 5e-3], q[0])[None]
    R, R0 = bn.quat_to_R(q[0]), bn.quat_to_R(qp[0])
    hh = np.array([[0.5 * L, 0.0, 0.0]])
    x, xp = x0.copy(), x0.copy()
    sel = [v for v in range(len(x0)) if abs(x0[v, 1] - mid[1]) < 1.01 * DX and abs(x0[v, 0] - mid[0]) < 0.5 * L + 1.01 * DX]
    for v in sel:
        P0 = bn.Pair(x0[v], x0[v], cp[0], R0, cp[0], R0, hh[0], rad, 0.0, 1.0, 1.0, 1.0)
        n0, b0 = P0.n, P0.b
        xp[v] = cp[0] + R0 @ b0 + (rad + rng.uniform(-0.5 * eps, 2.5 * eps)) * n0
        ang = rng.uniform(0, 2 * np.pi)
        t = np.array([np.cos(ang), np.sin(ang), 0.0]); t -= n0 * (n0 @ t); t /= np.linalg.norm(t)
        base = xp[v] + ((c[0] + R @ b0) - (cp[0] + R0 @ b0)) + rng.choice([0.0, 0.3 * eh, 3.0 * eh]) * t
        al, want = 0.0, rng.uniform(-0.5 * eps, 2.5 * eps)
        for _ in range(12):
            P = bn.Pair(base + al * n0, xp[v], c[0], R, cp[0], R0, hh[0], rad, 0.0, 1.0, 1.0, 1.0)
            al += (want - P.d) / max(float(P.n @ n0), 0.5)
        x[v] = base + al * n0
    mask = np.zeros(len(x0), np.uint8); mask[sel] = 1; mask[sel[2]] = 0
    return c, q, cp, qp, hh, np.array([rad]), np.array([0.5]), mask, x, xp


def _against(S, ctx, key_other):
    """energy, gradient and operator (spd 0 and 1) of the boxes alone against those of the other kind alone, each as the difference to neither; then
    both are left on for the read-outs"""
    def numbers(kb, ko):
        ctx.set_param("k_box", kb); ctx.set_param(key_other, ko)
        return [np.array(S.energy()), S.grad(), S.operator(0), S.operator(1)]

    base, box, other = numbers(0.0, 0.0), numbers(K, 0.0), numbers(0.0, K)
    for name, z, b, o in zip(("energy", "gradient", "operator spd 0", "operator spd 1"), base, box, other):
        db, do = b - z, o - z
        print("%s: box against %s %.2e of the largest entry" % (name, key_other, np.abs(db - do).max() / np.abs(do).max()))
        assert np.abs(do).max() > 0 and np.abs(db - do).max() <= 1e-12 * np.abs(do).max()
    ctx.set_param("k_box", K); ctx.set_param(key_other, K)


def test_a_box_with_half_extents_L2_0_0_is_the_rod_kernels():
    """the same state through the box kernels (h = (L/2, 0, 0)) and through the capsule kernels (a = c - (L/2) u, b = c + (L/2) u, likewise at the start
    of the step): energy, gradient, operator in both modes, force and torque (the rod's midpoint is the box's centre), and the pose-gradient
    identities g_c = g_a + g_b, g_th = (L/2) u x (g_b - g_a), likewise for the previous pose, mu and r as they are, to 1e-12 of the largest entry.
    The two share no launch."""
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    rng = np.random.default_rng(17)
    L = 4.008 * DX
    c, q, cp, qp, hh, rad, mu, mask, x, xp = _limit_state(s, rng, L)
    R, R0 = bn.quat_to_R(q[0]), bn.quat_to_R(qp[0])
    u, u0 = R[:, 0], R0[:, 0]
    a, b, ap, bp = c - 0.5 * L * u, c + 0.5 * L * u, cp - 0.5 * L * u0, cp + 0.5 * L * u0
    act, act0, reg, reg0 = bn.active_sets(x, xp, *_table(c, q, cp, qp, hh, mask, s.eps_contact, s.eps_v * s.dt, rad, mu))
    assert (act[:, 0] & act0[:, 0] & (reg[:, 0] == 1)).sum() >= 3 and (act[:, 0] & act0[:, 0] & (reg[:, 0] == 0)).sum() >= 1
    fz = _frozen_pattern(s.frozen.to_numpy().reshape(-1, 3), [30, 40, 50])
    ctx.set_frozen(fz.reshape(-1))
    ctx.set_boxes(c, q, hh, rad, mu, mask); ctx.set_box_poses(c, q, cp, qp)
    ctx.set_capsules(a, b, rad, mu, mask); ctx.set_capsule_ends(a, b, ap, bp)
    S = _State(ctx, x, xp, s._ref_angle)
    _against(S, ctx, "k_capsule")
    fb, fc = ctx.box_force(S.pos, S.prev), ctx.capsule_force(S.pos, S.prev)
    for lo, hi in FORCE_GROUPS:
        assert np.abs(fb - fc)[:, lo:hi].max() <= 1e-12 * np.abs(fc[:, lo:hi]).max()
    p = _dev(rng.normal(size=3 * s.tot_NV))
    gb, gc = ctx.box_grad(S.pos, S.prev, p)[0], ctx.capsule_grad(S.pos, S.prev, p)[0]
    want = np.concatenate([gc[0:3] + gc[3:6], 0.5 * L * np.cross(u, gc[3:6] - gc[0:3]), gc[6:9] + gc[9:12], 0.5 * L * np.cross(u0, gc[9:12] - gc[6:9]), gc[12:14]])
    # (the bound of a column group is taken on what is added: g_a and g_b cancel in g_c where the rod carries the sheet evenly)
    scale = np.concatenate([np.full(3, np.abs(gc[0:6]).max()), np.full(3, 0.5 * L * np.abs(gc[0:6]).max()), np.full(3, np.abs(gc[6:12]).max()),
                            np.full(3, 0.5 * L * np.abs(gc[6:12]).max()), np.abs(gc[12:14])])
    print("box_grad against the endpoint gradients, per entry, of the group's scale:", np.abs(gb - want) / scale)
    assert np.abs(gc).min() > 0 and (np.abs(gb - want) <= 1e-12 * scale).all()
    s._close_ctx()


def test_a_box_with_half_extents_zero_is_the_ball_kernels():
    """h = (0, 0, 0) against the sphere kernels on the same state: energy, gradient, operator in both modes, force; box_grad[:, 0:3], [:, 6:9], [:, 12],
    [:, 13] equal sphere_grad[:, 0:3], [:, 3:6], [:, 6], [:, 7] to 1e-12 of the largest entry, and a ball does not feel how it is turned."""
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    rng = np.random.default_rng(19)
    c, q, cp, qp, hh, rad, mu, mask, x, xp = _limit_state(s, rng, 0.0)
    fz = _frozen_pattern(s.frozen.to_numpy().reshape(-1, 3), [30, 40, 50])
    ctx.set_frozen(fz.reshape(-1))
    ctx.set_boxes(c, q, hh, rad, mu, mask); ctx.set_box_poses(c, q, cp, qp)
    ctx.set_spheres(c, rad, mu, mask); ctx.set_sphere_centres(c, cp)
    S = _State(ctx, x, xp, s._ref_angle)
    _against(S, ctx, "k_sphere")
    fb, fs = ctx.box_force(S.pos, S.prev), ctx.sphere_force(S.pos, S.prev)
    assert np.abs(fb[:, 0:3] - fs).max() <= 1e-12 * np.abs(fs).max()
    p = _dev(rng.normal(size=3 * s.tot_NV))
    gb, gs = ctx.box_grad(S.pos, S.prev, p), ctx.sphere_grad(S.pos, S.prev, p)
    big = np.abs(gs[:, 0:6]).max()
    assert np.abs(gb[:, 0:3] - gs[:, 0:3]).max() <= 1e-12 * big and np.abs(gb[:, 6:9] - gs[:, 3:6]).max() <= 1e-12 * big
    assert abs(gb[0, 12] - gs[0, 6]) <= 1e-12 * abs(gs[0, 6]) and abs(gb[0, 13] - gs[0, 7]) <= 1e-12 * abs(gs[0, 7])
    assert np.abs(gb[:, 3:6]).max() <= 1e-12 * big * 0.0106 and np.abs(gb[:, 9:12]).max() <= 1e-12 * big * 0.0106 and np.abs(gs).min() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ all classes at once
def test_handles_ties_planes_a_ball_a_rod_and_boxes_in_one_scene():
    """Scene_seam (two 8 x 8 cloths, nine ties) with vertex handles, two planes, a ball, a rod and two boxes: the energy of all six equals the sum of
    the restatements (the partials of every class lie where energy_async says), and the handle, tie, plane, ball and rod numbers keep their bits
    with boxes on"""
    from thinshelllab_amd.task_scene.Scene_seam import Scene
    s = Scene(cloth_size=DX * 8, N=8, k_tie=K, perturb=0.0, newton_cap=200)
    s.init_all()
    NV = s.tot_NV
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(21)
    hv = np.array([100, 5, 130, 77], np.int32); hw = np.array([1.0, 0.5, 2.0, 1.5])
    s.set_handles(hv, K, hw)
    ht = s.pos.to_numpy()[hv] + rng.normal(scale=1e-3, size=(4, 3))
    s.set_handle_targets(ht)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((NV, 3)))
    x0 = s.pos.to_numpy()
    first = np.arange(81)
    c, q, cp, qp, h, xp, x, near, near1 = pushed(x0, first, 8, eps, eh, seed=9)
    x[81:] += rng.normal(scale=2e-4, size=(NV - 81, 3))   # (the second cloth moves too: the seam is stretched)
    n = cn.unit([[0.0, 0.0, 1.0], [0.0, np.sin(0.3), np.cos(0.3)]])
    o = np.array([float(x0[:, 2].mean()), float(n[1] @ x0.mean(axis=0)) + 0.5 * eps])
    mu_p = np.array([0.5, 0.3])
    pmask = cn.full_mask(NV, 2); pmask[::7] = 1; pmask[3] = 0
    mid = x0.mean(axis=0)
    sc = np.array([[mid[0] - 0.01, mid[1] + 0.005, mid[2] - 1.0]]); scp = sc - [[0.4 * eh, 0.2 * eh, 0.6 * eh]]
    sR, smu = np.array([1.0]), np.array([0.4])
    smask = sn.full_mask(NV, 1); smask[::5] = 0
    ka = np.array([[mid[0] - 0.02, mid[1], mid[2] - 0.5]]); kb = np.array([[mid[0] + 0.02, mid[1] + 0.01, mid[2] - 0.5]])
    kap, kbp = ka - [[0.3 * eh, 0.1 * eh, 0.5 * eh]], kb - [[0.2 * eh, -0.3 * eh, 0.4 * eh]]
    kR, kmu = np.array([0.5]), np.array([0.3])
    kmask = kn.full_mask(NV, 1); kmask[::4] = 0
    bmask = _masks(NV, near, near1)
    idx, bb, w = tn.records(s.faces.to_numpy(), s._tie_v, s._tie_f, s._tie_b)
    S = _State(ctx, x, xp, s._ref_angle)
    fz = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_colliders(n, o, mu_p, pmask); ctx.set_param("k_collider", K)
    ctx.set_spheres(sc, sR, smu, smask); ctx.set_sphere_centres(sc, scp); ctx.set_param("k_sphere", K)
    ctx.set_capsules(ka, kb, kR, kmu, kmask); ctx.set_capsule_ends(ka, kb, kap, kbp); ctx.set_param("k_capsule", K)

    def numbers():
        p = _dev(np.random.default_rng(4).normal(size=3 * NV))
        return (ctx.handle_force(S.pos), ctx.handle_grad(p), ctx.tie_force(S.pos), ctx.tie_grad(S.pos, p), ctx.contact_blocks(False),
                ctx.collider_force(S.pos, S.prev), ctx.collider_grad(S.pos, S.prev, p), ctx.sphere_force(S.pos, S.prev), ctx.sphere_grad(S.pos, S.prev, p),
                ctx.capsule_force(S.pos, S.prev), ctx.capsule_grad(S.pos, S.prev, p), ctx.param_grads(S.pos, S.ref, ["k_handle", "k_tie"], p=p))
    S.operator(1)
    before = numbers()
    e_five, g_five = S.energy(), S.grad()
    keys = ("k_handle", "k_tie", "k_collider", "k_sphere", "k_capsule")
    for key in keys:
        ctx.set_param(key, 0.0)
    e_0 = S.energy()
    for key in keys:
        ctx.set_param(key, K)
    ctx.set_boxes(c, q, h, RAD, MU, bmask); ctx.set_box_poses(c, q, cp, qp); ctx.set_param("k_box", K)
    S.operator(1)
    after = numbers()
    for a, d in zip(before[:11], after[:11]):
        assert np.array_equal(a, d)
    assert before[11] == after[11] and ctx.tie_count() == 9 and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 9
    e_all, g_all = S.energy(), S.grad()
    e_h, e_t, e_c = hn.energy(x, hv, hw, ht, K), tn.energy(x, idx, bb, w, K), cn.energy(x, xp, n, o, mu_p, pmask, K, eps, eh)
    e_s = sn.energy(x, xp, sc, scp, sR, smu, smask, K, eps, eh)
    e_k = kn.energy(x, xp, ka, kb, kap, kbp, kR, kmu, kmask, K, eps, eh)
    A = _table(c, q, cp, qp, h, bmask, eps, eh)
    e_b = bn.energy(x, xp, *A)
    print("energy of the six classes %.17g, restatements %.17g + %.17g + %.17g + %.17g + %.17g + %.17g" % (e_all - e_0, e_h, e_t, e_c, e_s, e_k, e_b))
    tot = e_h + e_t + e_c + e_s + e_k + e_b
    assert min(e_h, e_t, e_c, e_s, e_k, e_b) > 1e-6 * tot          # (a class whose partials were lost or read twice would show a million times over the bound)
    assert abs((e_all - e_0) - (((((e_h + e_t) + e_c) + e_s) + e_k) + e_b)) <= 1e-12 * tot
    assert abs((e_all - e_five) - e_b) <= 1e-12 * tot
    gb = bn.gradient(x, xp, *A) * (fz == 0)
    assert np.abs((g_all - g_five) - gb).max() <= 1e-12 * max(np.abs(gb).max(), np.abs(g_all).max())
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ off means off
def _assemble_and_step(ctx, x, ref):
    pos = _dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, ref, spd=1, grad=F)
    H = ctx.operator_csr().toarray()
    e = ctx.energy(pos, prev, vel, ref)
    ctx.set_param("contact", 0.0)
    st = ctx.step(pos, prev, vel, ref)
    return F.cpu().numpy(), H, e, pos.cpu().numpy(), vel.cpu().numpy(), st["newton_iters"]


@pytest.mark.parametrize("how", ["removed", "k_zero"])
def test_off_means_off(how):
    rng = np.random.default_rng(5)
    fresh = _drape(12, perturb=1e-4)
    x = fresh.pos.to_numpy()
    y = x + rng.normal(scale=1e-4, size=x.shape) * (fresh.frozen.to_numpy().reshape(-1, 3) == 0)
    ctx_f = fresh._ensure_ctx()
    ctx_f.set_param("direct", 1)
    want = _assemble_and_step(ctx_f, y, fresh._ref_angle)
    used = _drape(12, perturb=1e-4)
    mid = x.mean(axis=0)
    used.set_boxes([[mid[0], mid[1], mid[2] - 0.012 - 1e-4], [mid[0] + 0.02, mid[1], mid[2] - 0.01]], [QID, _quat([0.0, 0.0, 0.5])], [[0.02, 0.01, 0.002], [0.005, 0.02, 0.0]],
                   [0.01, 0.01], [0.5, 0.2], 2000.0)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    used.move_boxes([[1e-5, 0.0, 1e-5], [1e-5, 1e-5, 1e-5]], [[0.0, 1e-3, 0.0], [1e-3, 0.0, 1e-3]])
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and ctx_u.box_count() == 2 and np.abs(used.box_force()).max() > 0
    assert not np.array_equal(_assemble_and_step(ctx_u, y, used._ref_angle)[0], want[0])
    if how == "removed":
        used.set_boxes([], [], [], [], [], 0.0)
        assert used._ensure_ctx() is ctx_u and ctx_u.box_count() == 0
    else:
        ctx_u.set_param("k_box", 0.0)
        f = ctx_u.box_force(_dev(y), _dev(y))
        g = ctx_u.box_grad(_dev(y), _dev(y), _dev(rng.normal(size=y.size)))
        assert ctx_u.box_count() == 2 and f.shape == (2, 6) and not f.any() and g.shape == (2, 14) and not g.any()
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    fresh._close_ctx(); used._close_ctx()


# ------------------------------------------------------------------------------------------------ whole rollouts
def _plate(N=8, **kw):
    from thinshelllab_amd.task_scene.Scene_table import Scene
    s = Scene(N=N, **kw)
    s.init_all()
    s._ensure_ctx().set_param("direct", 1)
    return s


STVK = (3.0e5, 2.0e5)
PLATE_PUSH, PLATE_K = 1.5e-3, 2.0e3
PLATE_ARM = 0.0105   # metres: half the plate's width, the scale that makes a rotation step comparable to a translation step
_RELAXED = {}


def _relaxed():
    """the rollout scene's start, computed once: the StVK sheet without bending (its matrix is the exact second derivative of its energy), all four
    corners frozen, pushed up on one side by Scene_table's plate whose rounded top lies 1.5 mm above the corners' plane, after 40 steps
    (positions, velocities)"""
    if not _RELAXED:
        s = _plate(Kb=0.0, stvk=STVK, push=PLATE_PUSH, k_box=PLATE_K, pin="all")
        for f in range(1, 41):
            assert s.time_step(None, f)["unconverged"] == 0
        _RELAXED["x"], _RELAXED["v"] = s.pos.to_numpy().copy(), s.vel.to_numpy().copy()
        s._close_ctx()
    return _RELAXED["x"].copy(), _RELAXED["v"].copy()


def _plate_trajectory(T, c0, q0, eh):
    """(centres (T, 1, 3), quaternions (T, 1, 4)): the plate rises a little, translates along x by 0.4, 1.6 and 2.8 eps_v dt and along y by 0.3 eps_v dt
    per step, and tilts about its long edge's direction and yaws so that its rim moves a further 0.6 eps_v dt per step; the slip per step
    straddles eps_v dt"""
    from thinshelllab_amd.engine import frames
    c, q = np.tile(c0, (T, 1, 1)), np.tile(q0, (T, 1, 1))
    for f in range(1, T):
        c[f], q[f] = frames.compose(c[f - 1], q[f - 1], [[(0.4 + 1.2 * (f - 1)) * eh, 0.3 * eh, 2e-6]], [[0.0, -0.3 * eh / PLATE_ARM, 0.6 * eh / PLATE_ARM]])
    return c, q


# The two difference steps of every check, a decade apart, as fractions of the parameter's own scale: those of tests/test_gpu_capsules.py -- a point
# of the plate and the start positions against the slip scale eps_v dt = 5e-5 m (2 % and 0.2 %; a rotation vector takes them over the plate's
# half width), the radius against the shell eps = 4e-4 m (2.5 % and 0.25 %), mu against mu = 0.5 (20 % and 2 %).  See there for why steps this
# size.
FD_STEPS = {"c": (1e-6, 1e-7), "th": (1e-6 / PLATE_ARM, 1e-7 / PLATE_ARM), "mu": (1e-1, 1e-2), "r": (1e-5, 1e-6), "x": (1e-6, 1e-7)}


def _rollout_checks(steps=FD_STEPS):
    """([(name, analytic, (difference at the larger step, at the smaller step))], smallest and largest slip of an active pair in one step of the tape in
    units of eps_v dt, per step the numbers of active vertices over (face, edge, corner))"""
    from thinshelllab_amd.engine import frames
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    x0, v0 = _relaxed()
    s = _plate(Kb=0.0, stvk=STVK, push=PLATE_PUSH, k_box=PLATE_K, pin="all")
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)
    c0, q0, h0, r0, mu0 = s.plate()
    c_traj, q_traj = _plate_trajectory(T, c0, q0, eh)
    mask = s._box_mask.copy()
    free = (s.frozen.to_numpy().reshape(-1, 3) == 0)
    sets = []

    def tables(c, q, r, mu):
        return [_table(c[fr], q[fr], c[fr - 1], q[fr - 1], h0, mask, eps, eh, r, mu, PLATE_K) for fr in range(1, T)]

    def rollout(c=c_traj, q=q_traj, mu=mu0, r=r0, x=x0, reverse=False):
        s.set_boxes(c[0], q[0], h0, r, mu, PLATE_K)
        # (row 0 of the tape is d(loss)/d(x_0) with the state before it held fixed: the start velocity moves with the start state)
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.from_numpy(v0 + (x - x0) * (s.damping / s.dt))
        g = Grad(s, T, 0); g.init_mass(s)
        g.count_kb_grad = False
        g.copy_pos(s, 0)
        for fr in range(1, T):
            s.set_box_poses(c[fr], q[fr])
            st = s.time_step(None, fr)
            assert st["unconverged"] == 0 and st["newton_iters"] < 50
            if reverse:
                print("step %d: %d Newton iterations, last delta %.2e" % (fr, st["newton_iters"], st["last_delta"]))
            g.copy_pos(s, fr)
        xs = g.pos_buffer.t.cpu().numpy()
        sets.append([bn.active_sets(xs[fr], xs[fr - 1], *A) for fr, A in zip(range(1, T), tables(c, q, r, mu))])
        L = float((xs[T - 1] * wgt).sum())
        if not reverse:
            return L
        assert np.array_equal(g.box_poses.t.numpy()[:, :, 0:3], c) and np.array_equal(g.box_poses_prev.t.numpy()[1:], g.box_poses.t.numpy()[:-1])
        g.pos_grad.t[T - 1] = _dev(wgt)
        for fr in range(T - 1, 0, -1):
            g.transfer_grad(fr, s, None)
            assert g.last_stats["flag"] != 3 and g.pos_grad.t[fr - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.box_grad.t.numpy().copy(), g.box_pose_grad().numpy().copy(), g.pos_grad.t[0].cpu().numpy().copy(), xs

    _, bg, pg, pg0, xs = rollout(reverse=True)
    assert bg.shape == (T, 1, 14) and pg.shape == (T, 1, 6) and (bg[0] == 0).all() and np.abs(bg[1:]).min() > 0
    assert np.array_equal(pg[:-1], bg[:-1, :, 0:6] + bg[1:, :, 6:12])
    slip = np.zeros((T - 1, len(x0)))
    for fr, A in zip(range(1, T), tables(c_traj, q_traj, r0, mu0)):
        for v, j, P in bn.pairs(xs[fr], xs[fr - 1], *A):
            slip[fr - 1, v] = P.r_w
    act = np.array([a[0][:, 0] & a[1][:, 0] for a in sets[0]])
    regions = [[int((act[fr] & (sets[0][fr][2][:, 0] == a)).sum()) for a in (2, 1, 0)] for fr in range(T - 1)]
    print("active vertices per step over (face, edge, corner): %s; slip per step of the active pairs: %.3e .. %.3e m, eps_v dt = %.1e m" % (regions, slip[act].min(), slip[act].max(), eh))
    d_c = rng.uniform(-1.0, 1.0, (T, 1, 3))
    d_th = rng.uniform(-1.0, 1.0, (T, 1, 3))
    d_mu = rng.uniform(0.5, 1.0, 1)
    d_r = rng.uniform(0.5, 1.0, 1)
    e = rng.normal(size=x0.shape) * free
    turned = lambda hh: np.array([frames.compose(c_traj[f], q_traj[f], np.zeros((1, 3)), hh * d_th[f])[1] for f in range(T)])
    fd = lambda f, hs: [(f(hh) - f(-hh)) / (2 * hh) for hh in hs]
    checks = [("box_pose_grad[:, :, 0:3] . delta_c", float((pg[:, :, 0:3] * d_c).sum()), fd(lambda hh: rollout(c=c_traj + hh * d_c), steps["c"])),
              ("box_pose_grad[:, :, 3:6] . delta_theta", float((pg[:, :, 3:6] * d_th).sum()), fd(lambda hh: rollout(q=turned(hh)), steps["th"])),
              ("box_grad[:, :, 12] . delta_mu", float((bg[:, :, 12].sum(axis=0) * d_mu).sum()), fd(lambda hh: rollout(mu=mu0 + hh * d_mu), steps["mu"])),
              ("box_grad[:, :, 13] . delta_r", float((bg[:, :, 13].sum(axis=0) * d_r).sum()), fd(lambda hh: rollout(r=r0 + hh * d_r), steps["r"])),
              ("pos_grad[0] . direction", float((pg0 * e).sum()), fd(lambda hh: rollout(x=x0 + hh * e), steps["x"]))]
    for i, a in enumerate(sets[1:]):
        for fr in range(T - 1):
            on = sets[0][fr][0] | sets[0][fr][1]
            assert np.array_equal(a[fr][0], sets[0][fr][0]) and np.array_equal(a[fr][1], sets[0][fr][1]), "a vertex crossed the shell between the runs: a badly chosen input (perturbed run %d)" % i
            assert np.array_equal(a[fr][2][on], sets[0][fr][2][on]) and np.array_equal(a[fr][3][on], sets[0][fr][3][on]), "an active pair crossed an edge line between the runs: a badly chosen input (perturbed run %d)" % i
    for name, got, d in checks:
        print("%s: analytic %.10e, differences %s" % (name, got, " / ".join("%.10e" % v for v in d)))
        print("    (the last two disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (abs(d[-2] - d[-1]) / abs(d[-1]), abs(got - d[-1]) / abs(d[-1]), 3 * abs(d[-2] - d[-1]) / abs(d[-1])))
    s._close_ctx()
    return checks, (slip[act].min() / eh, slip[act].max() / eh), regions


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last state; Scene_table with the
    StVK sheet without bending and four frozen corners, relaxed over the plate for 40 steps; the plate then rises by 2e-6 m per step, translates,
    tilts and yaws (_plate_trajectory).  box_pose_grad() contracted with a random centre-trajectory direction and with a random rotation-trajectory
    direction, the mu and r columns summed over the steps, and pos_grad[0] . e along a random free direction (the state before it held fixed),
    each against central differences at two steps a decade apart.  Bound: three times the disagreement of the two differences, which must itself
    be below 1e-2 of the value -- the rods' tape length, steps and bound.  No vertex may cross d = eps or d0 = eps, and no active pair may cross an
    edge line of the core box, between the runs.  Active vertices exist over the face and over the edge on every step.  The measured figures
    are in DESIGN.md 2.12."""
    checks, (slip_min, slip_max), regions = _rollout_checks()
    assert slip_max > 1.0 > slip_min > 2e-5          # both friction regimes on the tape (in units of eps_v dt; 2e-5: the r_w > 1e-9 switch of the block)
    for face, edge, corner in regions:
        assert face >= 1 and edge >= 1, regions
    for name, got, fd in checks:
        assert abs(fd[0] - fd[1]) < 1e-2 * abs(fd[1]), name
        assert abs(got - fd[1]) <= 3 * abs(fd[0] - fd[1]), name


# ------------------------------------------------------------------------------------------------ groups and plans
T_TAPE = 5


def _tape(s):
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    g = Grad(s, T_TAPE, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    return g


def test_group_members_equal_their_single_runs_and_two_runs_repeat():
    from thinshelllab_amd.scene_group import SceneGroup
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(81, 3))
    A, B = ((2e-5, 1e-5, 2e-6), (0.0, -1e-3, 2e-3)), ((-4e-5, 0.0, -1e-6), (1e-3, 1e-3, -2e-3))
    runs = {}
    for tag, (dp, dth) in (("a", A), ("b", A), ("c", B)):
        s = _plate(push=2e-4)
        g = _tape(s)
        for f in range(1, T_TAPE):
            s.move_boxes([dp], [dth])
            st = s.time_step(None, f)
            assert st["unconverged"] == 0 and st["factorizations"] > 0, st
            g.copy_pos(s, f)
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
        for f in range(T_TAPE - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.last_stats["flag"] != 3
        runs[tag] = (g.pos_buffer.t.cpu().numpy().copy(), g.pos_grad.t.cpu().numpy().copy(), g.box_grad.t.numpy().copy(), g.box_poses.t.numpy().copy())
        s._close_ctx()
    for a, d in zip(runs["a"], runs["b"]):
        assert np.array_equal(a, d)
    assert not np.array_equal(runs["a"][0], runs["c"][0]) and np.abs(runs["a"][2][1:, :, :12]).min() > 0 and (runs["a"][2][0] == 0).all()
    ms = [_plate(push=2e-4), _plate(push=2e-4)]
    G = SceneGroup(ms)
    gs = [_tape(m) for m in ms]
    for f in range(1, T_TAPE):
        for m, (dp, dth) in zip(ms, (A, B)):
            m.move_boxes([dp], [dth])
        sts = G.time_step(None, f)
        assert all(r["unconverged"] == 0 for r in sts)
        for m, g in zip(ms, gs):
            g.copy_pos(m, f)
    for g in gs:
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
    for f in range(T_TAPE - 1, 0, -1):
        G.transfer_grad(f, gs, None)
    assert G.info()["merged_factorizations"] > 0
    G.close()
    for i, tag in ((0, "a"), (1, "c")):
        for a in range(2):
            assert np.array_equal((gs[i].pos_buffer.t, gs[i].pos_grad.t)[a].cpu().numpy(), runs[tag][a]), (i, a)
        assert np.array_equal(gs[i].box_grad.t.numpy(), runs[tag][2]) and np.array_equal(gs[i].box_poses.t.numpy(), runs[tag][3]), i
        assert np.array_equal(gs[i].box_poses_prev.t.numpy()[1:], runs[tag][3][:-1])
    for m in ms:
        m._close_ctx()


def test_boxes_build_no_plan_and_no_slot():
    """the factorised path: the plan count after the first step does not change when boxes are switched on, over the rollout or in the reverse sweep"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    T = 4
    s = _plate(push=2e-4)
    c0, q0, h0, r0, mu0 = s.plate()
    s.set_boxes([], [], [], [], [], 0.0)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    st = s.time_step(None, 1)
    assert st["unconverged"] == 0 and st["factorizations"] > 0 and ctx.box_count() == 0
    plans = ctx.direct_info()["plans"]
    assert plans >= 1
    s.set_boxes(c0, q0, h0, r0, mu0, PLATE_K)
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    for f in range(1, T):
        s.move_boxes([[1e-5, -1e-5, 0.0]], [[0.0, 1e-3, 1e-3]])
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0 and st["nc"] == 0, st
        g.copy_pos(s, f)
        assert ctx.direct_info()["plans"] == plans and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 0
    assert s._ensure_ctx() is ctx and ctx.box_count() == 1 and np.abs(s.box_force()).max() > 0
    g.pos_grad.t[T - 1] = _dev(np.random.default_rng(7).normal(scale=1e-2, size=(s.tot_NV, 3)))
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3
    assert ctx.direct_info()["plans"] == plans and np.abs(g.box_grad.t.numpy()[1:]).max() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_keep_the_previous_list():
    s = _plate(push=2e-4)
    ctx = s._ensure_ctx()
    c0, q0, h0, r0, mu0 = s.plate()
    ctx.set_boxes(np.vstack([c0, c0 + [0.0, 0.0, -0.01]]), np.vstack([q0, q0]), np.vstack([h0, h0]), [r0[0], r0[0]], [0.5, 0.1])
    pos = _dev(s.pos.to_numpy())
    before = ctx.box_force(pos, pos)
    assert before.shape == (2, 6) and np.abs(before).max() > 0
    o, q1, hh = [0.0, 0.0, -1.0], [1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.5]
    cases = [(([o, [0.0, np.nan, 0.0]], [q1, q1], [hh, hh], [1.0, 1.0], [0.1, 0.1]), r"centre \(0, nan, 0\) of box 1 is not finite"),
             (([o, o], [q1, [0.0, 0.0, 0.0, 0.0]], [hh, hh], [1.0, 1.0], [0.1, 0.1]), r"quaternion \(0, 0, 0, 0\) of box 1 is zero or not finite"),
             (([o, o], [q1, [1.0, 0.0, np.inf, 0.0]], [hh, hh], [1.0, 1.0], [0.1, 0.1]), r"quaternion \(1, 0, inf, 0\) of box 1 is zero or not finite"),
             (([o, o], [q1, q1], [hh, [1.0, -1e-9, 1.0]], [1.0, 1.0], [0.1, 0.1]), r"half extents \(1, -1e-09, 1\) of box 1 are negative or not finite"),
             (([o, o], [q1, q1], [hh, hh], [1.0, 0.0], [0.1, 0.1]), r"radius 0 of box 1 is not finite and positive"),
             (([o, o], [q1, q1], [hh, hh], [1.0, np.inf], [0.1, 0.1]), r"radius inf of box 1 is not finite and positive"),
             (([o, o], [q1, q1], [hh, hh], [1.0, 1.0], [0.1, -0.5]), r"friction coefficient -0.5 of box 1 is negative or not finite"),
             (([o] * 9, [q1] * 9, [hh] * 9, [1.0] * 9, [0.1] * 9), r"9 boxes: at most 8")]
    for args, pat in cases:
        with pytest.raises(Exception, match="tsl_set_boxes: " + pat):
            ctx.set_boxes(*args)
        with pytest.raises(ValueError, match="set_boxes: " + pat):          # the scene's host check: the library's message
            s.set_boxes(*args, 10.0)
        assert ctx.box_count() == 2 and np.array_equal(ctx.box_force(pos, pos), before)
    bad = np.full(s.tot_NV, 3, np.uint8); bad[17] = 4
    with pytest.raises(Exception, match=r"tsl_set_boxes: mask 0x04 of vertex 17 names a box at or above 2"):
        ctx.set_boxes([o, o], [q1, q1], [hh, hh], [1.0, 1.0], [0.1, 0.1], bad)
    with pytest.raises(Exception, match=r"tsl_set_box_poses: centre \(inf, 0, -1\) of box 0 is not finite"):
        ctx.set_box_poses([[np.inf, 0.0, -1.0], o], [q1, q1])
    with pytest.raises(Exception, match=r"tsl_set_box_poses: quaternion \(0, 0, 0, 0\) of box 1 is zero or not finite"):
        ctx.set_box_poses([o, o], [q1, [0.0, 0.0, 0.0, 0.0]])
    with pytest.raises(Exception, match=r"tsl_set_box_poses: previous centre \(0, 0, nan\) of box 1 is not finite"):
        ctx.set_box_poses([o, o], [q1, q1], [o, [0.0, 0.0, np.nan]], [q1, q1])
    with pytest.raises(Exception, match=r"tsl_set_box_poses: previous quaternion \(nan, 0, 0, 0\) of box 0 is zero or not finite"):
        ctx.set_box_poses([o, o], [q1, q1], [o, o], [[np.nan, 0.0, 0.0, 0.0], q1])
    with pytest.raises(Exception, match=r"tsl_set_box_poses: previous centres without previous quaternions"):
        ctx.set_box_poses([o, o], [q1, q1], [o, o], None)
    with pytest.raises(Exception, match=r"tsl_set_box_poses: previous quaternions without previous centres"):
        ctx.set_box_poses([o, o], [q1, q1], None, [q1, q1])
    assert ctx.box_count() == 2 and np.array_equal(ctx.box_force(pos, pos), before)
    with pytest.raises(Exception, match="k_box must be finite and >= 0"):
        ctx.set_param("k_box", -1.0)
    with pytest.raises(Exception, match="k_box must be finite and >= 0"):
        ctx.set_param("k_box", np.nan)
    # eight are the most: accepted, and the list is the new one
    c8 = c0 + np.arange(8)[:, None] * [0.0002, 0.0005, 0.0]
    q8 = np.array([_quat([0.0, 0.0, 0.02 * j]) for j in range(8)])
    h8 = np.tile(h0, (8, 1))
    ctx.set_boxes(c8, q8, h8, [r0[0]] * 8, [0.1] * 8)
    cp8 = c8 - [2e-5, 1e-5, 1e-5]
    qp8 = np.array([_quat([1e-3, -2e-3, 1e-3], a) for a in q8])
    ctx.set_box_poses(c8, q8, cp8, qp8)
    prev = _dev(s.pos.to_numpy() - [1e-5, 2e-5, 0.0])
    f8 = ctx.box_force(pos, prev)
    assert ctx.box_count() == 8 and f8.shape == (8, 6) and np.abs(f8[:, 2]).min() > 0
    pn = np.random.default_rng(1).normal(size=(s.tot_NV, 3))
    g8 = ctx.box_grad(pos, prev, _dev(pn.reshape(-1)))
    A8 = _table(c8, q8, cp8, qp8, h8, bn.full_mask(s.tot_NV, 8), s.eps_contact, s.eps_v * s.dt, np.full(8, r0[0]), np.full(8, 0.1), s.k_box)
    g8_np = bn.box_grad(s.pos.to_numpy(), prev.cpu().numpy().reshape(-1, 3), pn, s.frozen.to_numpy().reshape(-1, 3), *A8)
    f8_np = bn.force(s.pos.to_numpy(), prev.cpu().numpy().reshape(-1, 3), *A8)
    assert g8.shape == (8, 14) and np.abs(g8_np).max() > 0
    for lo, hi in GRAD_GROUPS:
        assert np.abs(g8 - g8_np)[:, lo:hi].max() <= 1e-12 * np.abs(g8_np[:, lo:hi]).max(), (lo, hi)
    for lo, hi in FORCE_GROUPS:
        assert np.abs(f8 - f8_np)[:, lo:hi].max() <= 1e-12 * np.abs(f8_np[:, lo:hi]).max(), (lo, hi)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_table import optimise
    losses, cen, quat = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
    assert cen.shape == (4, 1, 3) and quat.shape == (4, 1, 4) and (cen[1:] != cen[0]).any() and (quat[1:] != quat[0]).any()
