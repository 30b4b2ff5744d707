"""Capsule colliders (tsl_set_capsules; csrc/k_capsule.hpp) through the C ABI.  The reference has no such term: it is checked
against the dense NumPy restatement (tests/capsule_numpy.py), the sphere colliders where a rod touches with one cap only, and whole-rollout
differences.  The idiom is that of tests/test_gpu_spheres.py: a capsule quantity of a state is the difference against the same state with
k_capsule = 0 -- no capsule kernel runs there, and the rest is formed by the same launches in both -- and K = 2e5 N/m, the size of the cloth's own
diagonal entries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import capsule_numpy as kn  # noqa: E402
import collider_numpy as cn  # noqa: E402
import handle_numpy as hn  # noqa: E402
import sphere_numpy as sn  # noqa: E402
import tie_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu

K = 2.0e5
DX = 0.1 / 15


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

    def part(self, fun, k=K, with_base=False, key="k_capsule"):
        """fun() with k_capsule = k minus fun() with k_capsule = 0 (with_base: and the latter)"""
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


RADII = np.array([1.0, 0.5])
MU = np.array([0.5, 0.3])


def _closest(p, a, b):
    e = b - a
    t = min(max(float((p - a) @ e) / float(e @ e), 0.0), 1.0)
    return a + t * e, t


def pushed(x0, sel, n_side, eps, eh, seed):
    """the vertices `sel` of a flat horizontal sheet (n_side cells of DX along x) pushed partly through two rods of radius 1 m and 0.5 m under it whose
    tops lie in the sheet, both of them translating, turning and changing length by about eps_v dt.  Rod 0 lies along x under the middle and is half
    as long as the sheet is wide, plus 0.008 DX: the vertex columns a quarter of the sheet from the middle lie 0.004 DX inside its ends, the ones
    beyond them over its caps.  Distances and start-of-step distances to rod 0 on either side of the shell independently, slips relative to the rod's
    material point of 0, 0.3 and 3 times eps_v dt (the last carries vertices of those columns from the barrel onto a cap); rod 1, along y a third of the
    sheet beside, its top half a shell higher, meets whatever heights that gives.  (a, b, ap, bp, x_prev, x)"""
    rng = np.random.default_rng(seed)
    x, xp = x0.copy(), x0.copy()
    mid = x0[sel].mean(axis=0)
    w = n_side * DX
    hl = (n_side / 4 + 0.004) * DX
    z0, z1 = mid[2] - RADII[0], mid[2] - RADII[1] + 0.5 * eps
    a = np.array([[mid[0] - hl, mid[1], z0], [mid[0] + w / 3, mid[1] - 0.3 * w, z1]])
    b = np.array([[mid[0] + hl, mid[1], z0], [mid[0] + w / 3, mid[1] + 0.3 * w, z1]])
    ap = a - np.array([[0.4 * eh, 0.2 * eh, 0.6 * eh], [-0.2 * eh, 0.4 * eh, 0.2 * eh]])
    bp = b - np.array([[0.3 * eh, -0.4 * eh, 0.5 * eh], [0.3 * eh, 0.2 * eh, -0.1 * eh]])
    # two vertices of each of those columns: inside both shells, 3 eps_v dt of slip along the axis and outwards -- t is clamped while t0 is not
    col = {int(v): ang for side, ang in ((-1.0, np.pi), (1.0, 0.0)) for v in [u for u in sel if abs(x0[u, 0] - (mid[0] + side * (n_side // 4) * DX)) < 1e-6 * DX][2:4]}
    for v in sel:
        c0, t0 = _closest(x0[v], ap[0], bp[0])
        n0 = (x0[v] - c0) / np.linalg.norm(x0[v] - c0)
        g0, slip, ang, want = rng.uniform(-0.5 * eps, 2.5 * eps), rng.choice([0.0, 0.3 * eh, 3.0 * eh]), rng.uniform(0, 2 * np.pi), rng.uniform(-0.5 * eps, 2.5 * eps)
        if int(v) in col:
            g0, slip, ang, want = 0.3 * eps, 3.0 * eh, col[int(v)], 0.2 * eps
        xp[v] = c0 + (RADII[0] + g0) * n0
        t = np.array([np.cos(ang), np.sin(ang), 0.0]); t -= n0 * (n0 @ t); t /= np.linalg.norm(t)
        base = xp[v] + ((1.0 - t0) * (a[0] - ap[0]) + t0 * (b[0] - bp[0])) + slip * t
        al = 0.0
        for _ in range(6):   # (the gap grows with the shift along n0 at a rate within 1e-6 of one)
            al += want - kn.Pair(base + al * n0, xp[v], a[0], b[0], ap[0], bp[0], RADII[0], 0.0, 1.0, 1.0, 1.0).d
        x[v] = base + al * n0
    return a, b, ap, bp, xp, x


def branches(x, xp, A, mu):
    """asserts that the state walks through every branch; returns the active set"""
    a, b, ap, bp, R, _, mask, k, eps, eh = A
    act, act0, reg, reg0 = kn.active_sets(x, xp, *A)
    on = reg != 9
    r = np.zeros(act.shape)
    for v, j, P in kn.pairs(x, xp, *A):
        r[v, j] = P.r
    fr = act0 & (mu[None, :] > 0)
    for ia in (True, False):
        for ib in (True, False):
            assert (on & (act == ia) & (act0 == ib)).any()
    assert (fr & (r < 1e-9)).any() and (fr & (r > 1e-9) & (r < eh)).any() and (fr & (r > eh)).any()
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any() and (mask == 0).any() and (on.sum(axis=1) == 1).any()
    both = act[:, 0] & fr[:, 0]
    for region in (-1, 0, 1):     # both caps and the barrel of rod 0 carry normal force and friction
        assert (both & (reg[:, 0] == region)).any() and (both & (reg0[:, 0] == region)).any(), region
    change = both & (reg[:, 0] != reg0[:, 0])
    print("pairs of rod 0 with normal force and friction: %d, of them over cap a / barrel / cap b %s, with t clamped while t0 is not %d, the other way round %d"
          % (both.sum(), [int((both & (reg[:, 0] == q)).sum()) for q in (-1, 0, 1)], (change & (reg0[:, 0] == 0)).sum(), (change & (reg[:, 0] == 0)).sum()))
    assert (change & (reg0[:, 0] == 0)).any()
    assert min(np.abs(a - ap).min(), np.abs(b - bp).min(), np.abs((b - bp) - (a - ap)).min()) > 0
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
    of the largest capsule entry (of each column group for the read-outs), the spheres' bound."""
    ctx = S.ctx
    NV = len(x)
    assert ctx.capsule_count() == len(A[0])
    e_np, g_np = kn.energy(x, xp, *A), kn.gradient(x, xp, *A)
    H_ex, H_pr = kn.hessian(x, xp, *A, exact=True), kn.hessian(x, xp, *A, exact=False)
    B_np = kn.blocks(x, xp, *A)
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
            print("%s: operator err / largest capsule entry %.2e, asymmetric entries of the difference / of the rest %d / %d"
                  % (tag, np.abs(D - Hm).max() / big, (D != D.T).sum(), (Ab != Ab.T).sum()))
            assert np.abs(D - Hm).max() <= 1e-12 * big
            assert (D[~inside] == 0).all() and (D[~free] == 0).all() and (D[:, ~free] == 0).all()
            assert not ((D != D.T) & (Ab == Ab.T)).any()
            got[tag] = (D, Ab)
        # spd 0 against spd 1: exactly the curvature term, which has lost the axis direction over the barrel
        curv = H_ex - H_pr
        cb = kn.curvature_blocks(x, xp, *A)
        for v in range(NV):
            assert np.abs(curv[3 * v:3 * v + 3, 3 * v:3 * v + 3] - cb[v]).max() <= 1e-12 * big
        dc = (got["spd 0"][0] - got["spd 1"][0]) - curv * ff
        print("spd 0 - spd 1 against the curvature term: %.2e of the largest capsule entry (the term itself %.2e)" % (np.abs(dc).max() / big, np.abs(curv * ff).max() / big))
        assert np.abs(dc).max() <= 1e-12 * big
        for tag in ("spd 2", "literal"):   # the projected modes add the same numbers: the same bits wherever the rest of the operator has the same bits
            D1, A1 = got["spd 1"]; D2, A2 = got[tag]
            same = (A1 == A2) & inside
            assert (D1[same] == D2[same]).all() and np.abs(D1 - D2).max() <= 1e-12 * big
        # the read-outs (frozen dofs: not masked in the force, not counted in the gradients)
        fo, fo_np = ctx.capsule_force(S.pos, S.prev), kn.force(x, xp, *A)
        pn = np.random.default_rng(11).normal(size=(NV, 3))
        cg, cg_np = ctx.capsule_grad(S.pos, S.prev, _dev(pn.reshape(-1))), kn.capsule_grad(x, xp, pn, frozen, *A)
        assert fo.shape == fo_np.shape == (len(A[0]), 6) and cg.shape == cg_np.shape == (len(A[0]), 14)
        for lo, hi in FORCE_GROUPS:
            print("  capsule_force[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(fo - fo_np)[:, lo:hi].max() / np.abs(fo_np[:, lo:hi]).max()))
            assert np.abs(fo - fo_np)[:, lo:hi].max() <= 1e-12 * np.abs(fo_np[:, lo:hi]).max()
        for lo, hi in GRAD_GROUPS:
            print("  capsule_grad[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(cg - cg_np)[:, lo:hi].max() / np.abs(cg_np[:, lo:hi]).max()))
            assert np.abs(cg - cg_np)[:, lo:hi].max() <= 1e-12 * np.abs(cg_np[:, lo:hi]).max()
        assert np.abs(cg_np).min() > 0 and np.abs(fo_np).min() > 0


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
    a, b, ap, bp, xp, x = pushed(s.pos.to_numpy(), np.arange(NV), N, eps, eh, seed=N)
    mask = kn.full_mask(NV, 2)
    mask[[3, 40]] = 0; mask[[5, 41, 50]] = 2; mask[[7, 60]] = 1
    A = (a, b, ap, bp, RADII, MU, mask, K, eps, eh)
    act = branches(x, xp, A, MU)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    assert fz0.any()
    ctx.set_capsules(a, b, RADII, MU, mask)
    ctx.set_capsule_ends(a, b, ap, bp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, x, xp, A, [fz0, _frozen_pattern(fz0, touched)])
    # new endpoints alone: the table follows; without previous endpoints the rods are at rest
    ctx.set_frozen(fz0.reshape(-1))
    a2, b2 = a + [[1e-4, 0.0, -2e-4], [0.0, 1e-4, 1e-4]], b + [[-1e-4, 1e-4, -1e-4], [1e-4, 0.0, 2e-4]]
    e_old = kn.energy(x, xp, *A)
    for pa, pb, qa, qb in ((ap, bp, ap, bp), (None, None, a2, b2)):
        ctx.set_capsule_ends(a2, b2, pa, pb)
        e = S.part(S.energy)
        e_np = kn.energy(x, xp, a2, b2, qa, qb, *A[4:])
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
    x0 = s.pos.to_numpy()
    NV = s.tot_NV
    cloth = np.arange(cl.offset, cl.offset + cl.NV)
    a, b, ap, bp, xp, x = pushed(x0, cloth, 8, eps, eh, seed=5)
    mask = np.zeros(NV, np.uint8)          # (the bodies see no capsule)
    mask[cloth] = 3; mask[cloth[[3, 40]]] = 0; mask[cloth[[5, 41, 50]]] = 2; mask[cloth[[7, 60]]] = 1
    A = (a, b, ap, bp, RADII, MU, mask, K, eps, eh)
    act = branches(x, xp, A, MU)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_capsules(a, b, RADII, MU, mask)
    ctx.set_capsule_ends(a, b, ap, bp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, x, xp, A, [fz0, _frozen_pattern(fz0, touched)])
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ a rod on end is a ball
def test_a_rod_on_end_is_the_ball_at_its_endpoint():
    """A rod of radius 1 m that stands on end under the sheet (b two metres below a, moving and tilting a little) touches it with the cap at a only:
    every active pair has t = t0 = 0.  On the same states the capsule kernels give what the sphere kernels give for a ball of the same radius and
    friction at a (previous centre ap) with k_sphere = k_capsule: energy, gradient, operator (spd 0 and 1), force to 1e-12 of the largest entry;
    capsule_grad[:, 0:3], [:, 6:9], [:, 12], [:, 13] equal sphere_grad[:, 0:3], [:, 3:6], [:, 6], [:, 7] within the same bound, and the b columns are
    exactly zero.  The two share no launch."""
    N = 8
    s = _drape(N)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    NV = s.tot_NV
    x0 = s.pos.to_numpy()
    rng = np.random.default_rng(17)
    mid = x0.mean(axis=0)
    R, mu = np.array([1.0]), np.array([0.5])
    a = np.array([[mid[0], mid[1], mid[2] - R[0]]])
    ap = a - [[0.4 * eh, 0.2 * eh, 0.6 * eh]]
    b = a - [[0.0, 0.0, 2.0]]
    bp = ap - [[2.0 * eh, -3.0 * eh, 2.0 + eh]]
    x, xp = x0.copy(), x0.copy()
    for v in range(NV):     # the state of the spheres' test: gaps on either side of the shell, slips of 0, 0.3 and 3 eps_v dt relative to the ball at a
        u0 = x0[v] - ap[0]; u0 /= np.linalg.norm(u0)
        xp[v] = ap[0] + (R[0] + rng.uniform(-0.5 * eps, 2.5 * eps)) * u0
        ang = rng.uniform(0, 2 * np.pi)
        t = np.array([np.cos(ang), np.sin(ang), 0.0]); t -= u0 * (u0 @ t); t /= np.linalg.norm(t)
        q = xp[v] + (a[0] - ap[0]) + rng.choice([0.0, 0.3 * eh, 3.0 * eh]) * t - a[0]
        x[v] = a[0] + (R[0] + rng.uniform(-0.5 * eps, 2.5 * eps)) * q / np.linalg.norm(q)
    mask = kn.full_mask(NV, 1); mask[[3, 40]] = 0
    A = (a, b, ap, bp, R, mu, mask, K, eps, eh)
    n_act = 0
    for v, j, P in kn.pairs(x, xp, *A):
        if P.act or P.act0:
            assert P.t == 0.0 and P.t0 == 0.0 and not P.inn and not P.in0
            n_act += 1
    assert n_act > 20
    fz = _frozen_pattern(s.frozen.to_numpy().reshape(-1, 3), [10, 30, 50])
    ctx.set_frozen(fz.reshape(-1))
    ctx.set_capsules(a, b, R, mu, mask); ctx.set_capsule_ends(a, b, ap, bp)
    ctx.set_spheres(a, R, mu, mask); ctx.set_sphere_centres(a, ap)
    S = _State(ctx, x, xp, s._ref_angle)
    p = _dev(rng.normal(size=3 * NV))

    def numbers(kc, ks):
        ctx.set_param("k_capsule", kc); ctx.set_param("k_sphere", ks)
        return [np.array(S.energy()), S.grad(), S.operator(0), S.operator(1)]

    base, cap, sph = numbers(0.0, 0.0), numbers(K, 0.0), numbers(0.0, K)
    for name, z, c, q in zip(("energy", "gradient", "operator spd 0", "operator spd 1"), base, cap, sph):
        dc, ds = c - z, q - z
        print("%s: capsule against sphere %.2e of the largest entry" % (name, np.abs(dc - ds).max() / np.abs(ds).max()))
        assert np.abs(ds).max() > 0 and np.abs(dc - ds).max() <= 1e-12 * np.abs(ds).max()
    ctx.set_param("k_capsule", K); ctx.set_param("k_sphere", K)
    fc, fs = ctx.capsule_force(S.pos, S.prev), ctx.sphere_force(S.pos, S.prev)
    assert np.abs(fc[:, 0:3] - fs).max() <= 1e-12 * np.abs(fs).max()
    gc, gs = ctx.capsule_grad(S.pos, S.prev, p), ctx.sphere_grad(S.pos, S.prev, p)
    big = np.abs(gs[:, 0:6]).max()
    print("capsule_grad against sphere_grad: a %.2e, ap %.2e of the largest entry; mu %.2e, R %.2e relative"
          % (np.abs(gc[:, 0:3] - gs[:, 0:3]).max() / big, np.abs(gc[:, 6:9] - gs[:, 3:6]).max() / big, abs(gc[0, 12] - gs[0, 6]) / abs(gs[0, 6]), abs(gc[0, 13] - gs[0, 7]) / abs(gs[0, 7])))
    assert np.abs(gc[:, 0:3] - gs[:, 0:3]).max() <= 1e-12 * big and np.abs(gc[:, 6:9] - gs[:, 3:6]).max() <= 1e-12 * big
    assert abs(gc[0, 12] - gs[0, 6]) <= 1e-12 * abs(gs[0, 6]) and abs(gc[0, 13] - gs[0, 7]) <= 1e-12 * abs(gs[0, 7])
    assert (gc[:, 3:6] == 0).all() and (gc[:, 9:12] == 0).all() and np.abs(gs).min() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ all classes at once
def test_handles_ties_planes_a_ball_and_a_rod_in_one_scene():
    """Scene_seam (two 8 x 8 cloths, nine ties) with vertex handles, two planes, a ball and two rods: the energy of all five equals the sum of the
    restatements (the partials of every class lie where energy_async says), and the handle, tie, plane and ball numbers keep their bits with capsules on"""
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
    a, b, ap, bp, xp, x = pushed(x0, np.arange(NV), 8, eps, eh, seed=9)
    n = cn.unit([[0.0, 0.0, 1.0], [0.0, np.sin(0.3), np.cos(0.3)]])
    o = np.array([float(x0[:, 2].mean()), float(n[1] @ x0.mean(axis=0)) + 0.5 * eps])
    mu_p = np.array([0.5, 0.3])
    pmask = cn.full_mask(NV, 2); pmask[::7] = 1; pmask[3] = 0
    mid = x0.mean(axis=0)
    sc = np.array([[mid[0] - 0.01, mid[1] + 0.005, mid[2] - 1.0]]); scp = sc - [[0.4 * eh, 0.2 * eh, 0.6 * eh]]
    sR, smu = np.array([1.0]), np.array([0.4])
    smask = sn.full_mask(NV, 1); smask[::5] = 0
    kmask = kn.full_mask(NV, 2); kmask[::5] = 2; kmask[4] = 0
    idx, bb, w = tn.records(s.faces.to_numpy(), s._tie_v, s._tie_f, s._tie_b)
    S = _State(ctx, x, xp, s._ref_angle)
    fz = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_colliders(n, o, mu_p, pmask); ctx.set_param("k_collider", K)
    ctx.set_spheres(sc, sR, smu, smask); ctx.set_sphere_centres(sc, scp); ctx.set_param("k_sphere", K)

    def numbers():
        p = _dev(np.random.default_rng(4).normal(size=3 * NV))
        return (ctx.handle_force(S.pos), ctx.handle_grad(p), ctx.tie_force(S.pos), ctx.tie_grad(S.pos, p), ctx.contact_blocks(False),
                ctx.collider_force(S.pos, S.prev), ctx.collider_grad(S.pos, S.prev, p), ctx.sphere_force(S.pos, S.prev), ctx.sphere_grad(S.pos, S.prev, p),
                ctx.param_grads(S.pos, S.ref, ["k_handle", "k_tie"], p=p))
    S.operator(1)
    before = numbers()
    e_four, g_four = S.energy(), S.grad()
    for key in ("k_handle", "k_tie", "k_collider", "k_sphere"):
        ctx.set_param(key, 0.0)
    e_0 = S.energy()
    for key in ("k_handle", "k_tie", "k_collider", "k_sphere"):
        ctx.set_param(key, K)
    ctx.set_capsules(a, b, RADII, MU, kmask); ctx.set_capsule_ends(a, b, ap, bp); ctx.set_param("k_capsule", K)
    S.operator(1)
    after = numbers()
    for q, d in zip(before[:9], after[:9]):
        assert np.array_equal(q, d)
    assert before[9] == after[9] and ctx.tie_count() == 9 and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 9
    e_all, g_all = S.energy(), S.grad()
    e_h, e_t, e_c = hn.energy(x, hv, hw, ht, K), tn.energy(x, idx, bb, w, K), cn.energy(x, xp, n, o, mu_p, pmask, K, eps, eh)
    e_s = sn.energy(x, xp, sc, scp, sR, smu, smask, K, eps, eh)
    A = (a, b, ap, bp, RADII, MU, kmask, K, eps, eh)
    e_k = kn.energy(x, xp, *A)
    print("energy of the five classes %.17g, restatements %.17g + %.17g + %.17g + %.17g + %.17g" % (e_all - e_0, e_h, e_t, e_c, e_s, e_k))
    tot = e_h + e_t + e_c + e_s + e_k
    assert min(e_h, e_t, e_c, e_s, e_k) > 1e-6 * tot          # (a class whose partials were lost or read twice would show a million times over the bound)
    assert abs((e_all - e_0) - ((((e_h + e_t) + e_c) + e_s) + e_k)) <= 1e-12 * tot
    assert abs((e_all - e_four) - e_k) <= 1e-12 * tot
    gk = kn.gradient(x, xp, *A) * (fz == 0)
    assert np.abs((g_all - g_four) - gk).max() <= 1e-12 * max(np.abs(gk).max(), np.abs(g_all).max())
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
    used.set_capsules([[mid[0] - 0.02, mid[1], -0.05 - 1e-4], [mid[0] + 0.02, mid[1] - 0.01, -0.02]], [[mid[0] + 0.02, mid[1], -0.05 - 1e-4], [mid[0] + 0.02, mid[1] + 0.01, -0.02]],
                      [0.05, 0.02], [0.5, 0.2], 2000.0)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    used.set_capsule_ends(used._cap_e[:, 0] + [1e-5, 0.0, 1e-5], used._cap_e[:, 1] + [1e-5, 1e-5, 1e-5])
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and ctx_u.capsule_count() == 2 and np.abs(used.capsule_force()).max() > 0
    assert not np.array_equal(_assemble_and_step(ctx_u, y, used._ref_angle)[0], want[0])
    if how == "removed":
        used.set_capsules([], [], [], [], 0.0)
        assert used._ensure_ctx() is ctx_u and ctx_u.capsule_count() == 0
    else:
        ctx_u.set_param("k_capsule", 0.0)
        f = ctx_u.capsule_force(_dev(y), _dev(y))
        g = ctx_u.capsule_grad(_dev(y), _dev(y), _dev(rng.normal(size=y.size)))
        assert ctx_u.capsule_count() == 2 and f.shape == (2, 6) and not f.any() and g.shape == (2, 14) and not g.any()
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for q, c in zip(want, got):
        assert np.array_equal(q, c)
    fresh._close_ctx(); used._close_ctx()


# ------------------------------------------------------------------------------------------------ a rod that turns
def _rod(N=8, **kw):
    from thinshelllab_amd.task_scene.Scene_rod import Scene
    s = Scene(N=N, **kw)
    s.init_all()
    s._ensure_ctx().set_param("direct", 1)
    return s


def _swept(mu, yaw):
    """Scene_rod, N = 8, 12 steps; yaw: the ends move eps_v dt per step along -y (a) and +y (b); else both move along +y.  (mean y displacement of the
    active vertices near end a, near end b, numbers of those vertices, the ends' total motion)"""
    s = _rod(mu=mu, push=2e-4)
    x0 = s.pos.to_numpy()
    step = s.eps_v * s.dt
    a0, b0, R, _ = s.rod()
    for f in range(1, 13):
        s.set_capsule_ends(a0 + [[0.0, (-step if yaw else step) * f, 0.0]], b0 + [[0.0, step * f, 0.0]])
        assert s.time_step(None, f)["unconverged"] == 0
    x = s.pos.to_numpy()
    A = (s._cap_ep[:, 0], s._cap_ep[:, 1], s._cap_ep_step[:, 0], s._cap_ep_step[:, 1], R, np.array([mu]), s._cap_mask, s.k_capsule, s.eps_contact, step)
    near = {0: [], 1: []}
    for v, j, P in kn.pairs(x, s.prev_pos.to_numpy(), *A):
        if P.act and (P.s < 0.25 or P.s > 0.75):
            near[int(P.s > 0.5)].append(v)
    s._close_ctx()
    dy = (x - x0)[:, 1]
    return float(dy[near[0]].mean()), float(dy[near[1]].mean()), (len(near[0]), len(near[1])), 12 * step


def test_a_rod_that_turns_drags_its_two_ends_opposite_ways():
    """the rod yaws about its midpoint: with mu = 0.5 the sheet near end a follows -y and near end b follows +y; with mu = 0 neither moves more than the
    sheet over a rod that translates along y without friction (every point of that rod moves eps_v dt per step, a point at t of the yawing one
    |2 t - 1| eps_v dt: what the moving normals alone do is largest there).  The dragged fractions are printed, not asserted."""
    ya, yb, n, moved = _swept(0.5, True)
    print("mu 0.5, yaw: %s active vertices near the ends, mean y displacement %.3e / %.3e m, the ends moved -/+ %.3e m: dragged fractions %.3f / %.3f" % (n, ya, yb, moved, -ya / moved, yb / moved))
    assert min(n) >= 1 and ya < 0 < yb
    ta, tb, _, _ = _swept(0.0, False)
    bound = max(abs(ta), abs(tb))
    za, zb, n0, _ = _swept(0.0, True)
    print("mu 0: yaw %.3e / %.3e m; translation %.3e / %.3e m, the bound %.3e m" % (za, zb, ta, tb, bound))
    assert min(n0) >= 1 and max(abs(za), abs(zb)) <= bound and max(abs(za), abs(zb)) < min(-ya, yb)


# ------------------------------------------------------------------------------------------------ whole rollouts
STVK = (3.0e5, 2.0e5)
ROD_PUSH, ROD_K = 1.5e-3, 2.0e3
_RELAXED = {}


def _relaxed():
    """the rollout scene's start, computed once: the StVK sheet without bending (its matrix is the exact second derivative of its energy), corners
    frozen, pushed up in the middle by Scene_rod's rod whose top lies 1.5 mm above the corners' plane, after 40 steps (positions, velocities)"""
    if not _RELAXED:
        s = _rod(Kb=0.0, stvk=STVK, push=ROD_PUSH, k_capsule=ROD_K)
        for f in range(1, 41):
            assert s.time_step(None, f)["unconverged"] == 0
        _RELAXED["x"], _RELAXED["v"] = s.pos.to_numpy().copy(), s.vel.to_numpy().copy()
        s._close_ctx()
    return _RELAXED["x"].copy(), _RELAXED["v"].copy()


def _rod_trajectory(T, e0, eh):
    """(T, 1, 2, 3): the rod rises a little, translates along x by 0.4, 1.6 and 2.8 eps_v dt and along y by 0.3 eps_v dt per step, and yaws: its ends
    move a further 0.6 eps_v dt per step along -y (a) and +y (b); the slip per step straddles eps_v dt"""
    e = np.tile(e0, (T, 1, 1, 1))
    for f in range(1, T):
        e[f, 0] = e[f - 1, 0] + [(0.4 + 1.2 * (f - 1)) * eh, 0.3 * eh, 2e-6]
        e[f, 0, 0, 1] -= 0.6 * eh; e[f, 0, 1, 1] += 0.6 * eh
    return e


# The two difference steps of every check, a decade apart, as fractions of the parameter's own scale, as in tests/test_gpu_spheres.py: endpoints and
# start positions against the slip scale eps_v dt = 5e-5 m (2 % and 0.2 %), the radius against the shell eps = 4e-4 m (2.5 % and 0.25 %), mu against
# mu = 0.5 (20 % and 2 %).  The differences are those of the time stepper as it is, whose Newton iteration stops at |p|max / dt < 1e-7: they
# differentiate an iterate a little away from the stationary point that the reverse step assumes, and steps this size keep the differences' own
# disagreement above that.
FD_STEPS = {"e": (1e-6, 1e-7), "mu": (1e-1, 1e-2), "R": (1e-5, 1e-6), "x": (1e-6, 1e-7)}


def _rollout_checks(steps=FD_STEPS):
    """([(name, analytic, (difference at the larger step, at the smaller step))], smallest and largest slip of an active pair in one step of the tape in
    units of eps_v dt, per step the numbers of active vertices over (cap a, barrel, cap b))"""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    x0, v0 = _relaxed()
    s = _rod(Kb=0.0, stvk=STVK, push=ROD_PUSH, k_capsule=ROD_K)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)
    a0, b0, R0, mu0 = s.rod()
    e_traj = _rod_trajectory(T, np.stack([a0, b0], axis=1), eh)
    mask = s._cap_mask.copy()
    free = (s.frozen.to_numpy().reshape(-1, 3) == 0)
    sets = []

    def tape_sets(xs, e, R, mu):
        return [kn.active_sets(xs[fr], xs[fr - 1], e[fr, :, 0], e[fr, :, 1], e[fr - 1, :, 0], e[fr - 1, :, 1], R, mu, mask, ROD_K, eps, eh) for fr in range(1, T)]

    def rollout(e=e_traj, mu=mu0, R=R0, x=x0, reverse=False):
        s.set_capsules(e[0, :, 0], e[0, :, 1], R, mu, ROD_K)
        # (row 0 of the tape is d(loss)/d(x_0) with the state before it held fixed: the start velocity moves with the start state)
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.from_numpy(v0 + (x - x0) * (s.damping / s.dt))
        g = Grad(s, T, 0); g.init_mass(s)
        g.count_kb_grad = False
        g.copy_pos(s, 0)
        for fr in range(1, T):
            s.set_capsule_ends(e[fr, :, 0], e[fr, :, 1])
            st = s.time_step(None, fr)
            assert st["unconverged"] == 0 and st["newton_iters"] < 50
            if reverse:
                print("step %d: %d Newton iterations, last delta %.2e" % (fr, st["newton_iters"], st["last_delta"]))
            g.copy_pos(s, fr)
        xs = g.pos_buffer.t.cpu().numpy()
        sets.append(tape_sets(xs, e, R, mu))
        L = float((xs[T - 1] * wgt).sum())
        if not reverse:
            return L
        assert np.array_equal(g.capsule_ends.t.numpy(), e) and np.array_equal(g.capsule_ends_prev.t.numpy()[1:], e[:-1])
        g.pos_grad.t[T - 1] = _dev(wgt)
        for fr in range(T - 1, 0, -1):
            g.transfer_grad(fr, s, None)
            assert g.last_stats["flag"] != 3 and g.pos_grad.t[fr - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.capsule_grad.t.numpy().copy(), g.capsule_end_grad().numpy().copy(), g.pos_grad.t[0].cpu().numpy().copy(), xs

    _, cg, eg, pg0, xs = rollout(reverse=True)
    assert cg.shape == (T, 1, 14) and eg.shape == (T, 1, 2, 3) and (cg[0] == 0).all() and np.abs(cg[1:]).min() > 0
    assert np.array_equal(eg[:-1].reshape(T - 1, 1, 6), cg[:-1, :, 0:6] + cg[1:, :, 6:12])
    slip = np.zeros((T - 1, len(x0)))
    for fr in range(1, T):
        for v, j, P in kn.pairs(xs[fr], xs[fr - 1], e_traj[fr, :, 0], e_traj[fr, :, 1], e_traj[fr - 1, :, 0], e_traj[fr - 1, :, 1], R0, mu0, mask, ROD_K, eps, eh):
            slip[fr - 1, v] = P.r
    act = np.array([q[0][:, 0] & q[1][:, 0] for q in sets[0]])
    regions = [[int((act[fr] & (sets[0][fr][2][:, 0] == q)).sum()) for q in (-1, 0, 1)] for fr in range(T - 1)]
    print("active vertices per step over (cap a, barrel, cap b): %s; slip per step of the active pairs: %.3e .. %.3e m, eps_v dt = %.1e m" % (regions, slip[act].min(), slip[act].max(), eh))
    d_e = rng.uniform(-1.0, 1.0, (T, 1, 2, 3))
    d_mu = rng.uniform(0.5, 1.0, 1)
    d_R = rng.uniform(0.5, 1.0, 1)
    e = rng.normal(size=x0.shape) * free
    fd = lambda f, hs: [(f(h) - f(-h)) / (2 * h) for h in hs]
    checks = [("capsule_end_grad . delta_e", float((eg * d_e).sum()), fd(lambda h: rollout(e=e_traj + h * d_e), steps["e"])),
              ("capsule_grad[:, :, 12] . delta_mu", float((cg[:, :, 12].sum(axis=0) * d_mu).sum()), fd(lambda h: rollout(mu=mu0 + h * d_mu), steps["mu"])),
              ("capsule_grad[:, :, 13] . delta_R", float((cg[:, :, 13].sum(axis=0) * d_R).sum()), fd(lambda h: rollout(R=R0 + h * d_R), steps["R"])),
              ("pos_grad[0] . direction", float((pg0 * e).sum()), fd(lambda h: rollout(x=x0 + h * e), steps["x"]))]
    for i, q in enumerate(sets[1:]):
        for fr in range(T - 1):
            on = sets[0][fr][0] | sets[0][fr][1]
            assert np.array_equal(q[fr][0], sets[0][fr][0]) and np.array_equal(q[fr][1], sets[0][fr][1]), "a vertex crossed the shell between the runs: a badly chosen input (perturbed run %d)" % i
            assert np.array_equal(q[fr][2][on], sets[0][fr][2][on]) and np.array_equal(q[fr][3][on], sets[0][fr][3][on]), "an active pair changed between a cap and the barrel between the runs: a badly chosen input (perturbed run %d)" % i
    for name, got, d in checks:
        print("%s: analytic %.10e, differences %s" % (name, got, " / ".join("%.10e" % v for v in d)))
        print("    (the last two disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (abs(d[-2] - d[-1]) / abs(d[-1]), abs(got - d[-1]) / abs(d[-1]), 3 * abs(d[-2] - d[-1]) / abs(d[-1])))
    s._close_ctx()
    return checks, (slip[act].min() / eh, slip[act].max() / eh), regions


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last state; Scene_rod with the
    StVK sheet without bending, relaxed over the rod for 40 steps; the rod then rises by 2e-6 m, translates and yaws (_rod_trajectory).
    capsule_end_grad() contracted with a random endpoint-trajectory direction, the mu and R columns summed over the steps, and pos_grad[0] . e along
    a random free direction (the state before it held fixed), each against central differences at two steps a decade apart.  Bound: three times the
    disagreement of the two differences, which must itself be below 1e-2 of the value.  No vertex may cross d = eps or d0 = eps, and no active pair
    may change between a cap and the barrel, between the runs.  Active vertices exist over the barrel and over a cap on every step.  The measured
    figures are in DESIGN.md 2.10."""
    checks, (slip_min, slip_max), regions = _rollout_checks()
    assert slip_max > 1.0 > slip_min > 2e-5          # both friction regimes on the tape (in units of eps_v dt; 2e-5: the r > 1e-9 switch of the block)
    for ca, ba, cb in regions:
        assert ba >= 1 and max(ca, cb) >= 1, regions
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


def _moving(shift_a, shift_b):
    s = _rod(push=2e-4)
    a0, b0 = s.rod()[:2]
    return s, (lambda f: (a0 + np.asarray(shift_a) * f, b0 + np.asarray(shift_b) * f))


def test_group_members_equal_their_single_runs_and_two_runs_repeat():
    from thinshelllab_amd.scene_group import SceneGroup
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(81, 3))
    A, B = ((2e-5, 1e-5, 2e-6), (2e-5, -2e-5, 2e-6)), ((-4e-5, 0.0, -1e-6), (-3e-5, 3e-5, 1e-6))
    runs = {}
    for tag, shift in (("a", A), ("b", A), ("c", B)):
        s, e_of = _moving(*shift)
        g = _tape(s)
        for f in range(1, T_TAPE):
            s.set_capsule_ends(*e_of(f))
            st = s.time_step(None, f)
            assert st["unconverged"] == 0 and st["factorizations"] > 0, st
            g.copy_pos(s, f)
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
        for f in range(T_TAPE - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.last_stats["flag"] != 3
        runs[tag] = (g.pos_buffer.t.cpu().numpy().copy(), g.pos_grad.t.cpu().numpy().copy(), g.capsule_grad.t.numpy().copy(), g.capsule_ends.t.numpy().copy())
        s._close_ctx()
    for q, d in zip(runs["a"], runs["b"]):
        assert np.array_equal(q, d)
    assert not np.array_equal(runs["a"][0], runs["c"][0]) and np.abs(runs["a"][2][1:, :, :12]).min() > 0 and (runs["a"][2][0] == 0).all()
    members = [_moving(*A), _moving(*B)]
    ms = [m[0] for m in members]
    G = SceneGroup(ms)
    gs = [_tape(m) for m in ms]
    for f in range(1, T_TAPE):
        for m, e_of in members:
            m.set_capsule_ends(*e_of(f))
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
        for q in range(2):
            assert np.array_equal((gs[i].pos_buffer.t, gs[i].pos_grad.t)[q].cpu().numpy(), runs[tag][q]), (i, q)
        assert np.array_equal(gs[i].capsule_grad.t.numpy(), runs[tag][2]) and np.array_equal(gs[i].capsule_ends.t.numpy(), runs[tag][3]), i
        assert np.array_equal(gs[i].capsule_ends_prev.t.numpy()[1:], runs[tag][3][:-1])
    for m in ms:
        m._close_ctx()


def test_capsules_build_no_plan_and_no_slot():
    """the factorised path: the plan count after the first step does not change when capsules are switched on, over the rollout or in the reverse sweep"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    T = 4
    s = _rod(push=2e-4)
    a0, b0, radius, mu = s.rod()
    s.set_capsules([], [], [], [], 0.0)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    st = s.time_step(None, 1)
    assert st["unconverged"] == 0 and st["factorizations"] > 0 and ctx.capsule_count() == 0
    plans = ctx.direct_info()["plans"]
    assert plans >= 1
    s.set_capsules(a0, b0, radius, mu, ROD_K)
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    for f in range(1, T):
        s.set_capsule_ends(a0 + [[1e-5 * f, -1e-5 * f, 0.0]], b0 + [[1e-5 * f, 1e-5 * f, 0.0]])
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0 and st["nc"] == 0, st
        g.copy_pos(s, f)
        assert ctx.direct_info()["plans"] == plans and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 0
    assert s._ensure_ctx() is ctx and ctx.capsule_count() == 1 and np.abs(s.capsule_force()).max() > 0
    g.pos_grad.t[T - 1] = _dev(np.random.default_rng(7).normal(scale=1e-2, size=(s.tot_NV, 3)))
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3
    assert ctx.direct_info()["plans"] == plans and np.abs(g.capsule_grad.t.numpy()[1:]).max() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_keep_the_previous_list():
    s = _rod(push=2e-4)
    ctx = s._ensure_ctx()
    a0, b0, R0, mu0 = s.rod()
    R = float(R0[0])
    ctx.set_capsules(np.vstack([a0, a0 + [0.0, 0.01, 0.0]]), np.vstack([b0, b0 + [0.0, 0.01, 0.0]]), [R, R], [0.5, 0.1])
    pos = _dev(s.pos.to_numpy())
    before = ctx.capsule_force(pos, pos)
    assert before.shape == (2, 6) and np.abs(before).max() > 0
    o, o1 = [0.0, 0.0, -1.0], [1.0, 0.0, -1.0]
    cases = [(([o, [0.0, np.nan, 0.0]], [o1, o1], [1.0, 1.0], [0.1, 0.1]), r"endpoint a \(0, nan, 0\) of capsule 1 is not finite"),
             (([o, o], [o1, [np.inf, 0.0, 0.0]], [1.0, 1.0], [0.1, 0.1]), r"endpoint b \(inf, 0, 0\) of capsule 1 is not finite"),
             (([o, o], [o1, [0.0, 5e-10, -1.0]], [1.0, 1.0], [0.1, 0.1]), r"segment of capsule 1 is 5e-10 m long: at least 1e-09 m"),
             (([o, o], [o1, o1], [1.0, 0.0], [0.1, 0.1]), r"radius 0 of capsule 1 is not finite and positive"),
             (([o, o], [o1, o1], [1.0, np.inf], [0.1, 0.1]), r"radius inf of capsule 1 is not finite and positive"),
             (([o, o], [o1, o1], [1.0, 1.0], [0.1, -0.5]), r"friction coefficient -0.5 of capsule 1 is negative or not finite"),
             (([o] * 9, [o1] * 9, [1.0] * 9, [0.1] * 9), r"9 capsules: at most 8")]
    for args, pat in cases:
        with pytest.raises(Exception, match="tsl_set_capsules: " + pat):
            ctx.set_capsules(*args)
        with pytest.raises(ValueError, match="set_capsules: " + pat):          # the scene's host check: the library's message
            s.set_capsules(*args, 10.0)
        assert ctx.capsule_count() == 2 and np.array_equal(ctx.capsule_force(pos, pos), before)
    bad = np.full(s.tot_NV, 3, np.uint8); bad[17] = 4
    with pytest.raises(Exception, match=r"tsl_set_capsules: mask 0x04 of vertex 17 names a capsule at or above 2"):
        ctx.set_capsules([o, o], [o1, o1], [1.0, 1.0], [0.1, 0.1], bad)
    with pytest.raises(Exception, match=r"tsl_set_capsule_ends: endpoint a \(inf, 0, -1\) of capsule 0 is not finite"):
        ctx.set_capsule_ends([[np.inf, 0.0, -1.0], o], [o1, o1])
    with pytest.raises(Exception, match=r"tsl_set_capsule_ends: segment of capsule 1 is 0 m long: at least 1e-09 m"):
        ctx.set_capsule_ends([o, o], [o1, o])
    with pytest.raises(Exception, match=r"tsl_set_capsule_ends: previous endpoint b \(0, 0, nan\) of capsule 1 is not finite"):
        ctx.set_capsule_ends([o, o], [o1, o1], [o, o], [o1, [0.0, 0.0, np.nan]])
    with pytest.raises(Exception, match=r"tsl_set_capsule_ends: previous segment of capsule 0 is 0 m long: at least 1e-09 m"):
        ctx.set_capsule_ends([o, o], [o1, o1], [o1, o], [o1, o1])
    with pytest.raises(Exception, match=r"tsl_set_capsule_ends: previous endpoints a without previous endpoints b"):
        ctx.set_capsule_ends([o, o], [o1, o1], [o, o], None)
    with pytest.raises(Exception, match=r"tsl_set_capsule_ends: previous endpoints b without previous endpoints a"):
        ctx.set_capsule_ends([o, o], [o1, o1], None, [o1, o1])
    assert ctx.capsule_count() == 2 and np.array_equal(ctx.capsule_force(pos, pos), before)
    with pytest.raises(Exception, match="k_capsule must be finite and >= 0"):
        ctx.set_param("k_capsule", -1.0)
    with pytest.raises(Exception, match="k_capsule must be finite and >= 0"):
        ctx.set_param("k_capsule", np.nan)
    # eight are the most: accepted, and the list is the new one
    a8 = a0 + np.arange(8)[:, None] * [0.0, 0.002, 0.0]
    b8 = b0 + np.arange(8)[:, None] * [0.0, 0.002, 0.0]
    ctx.set_capsules(a8, b8, [R] * 8, [0.1] * 8)
    ap8, bp8 = a8 - [2e-5, 1e-5, 1e-5], b8 - [1e-5, -2e-5, 2e-5]
    ctx.set_capsule_ends(a8, b8, ap8, bp8)
    prev = _dev(s.pos.to_numpy() - [1e-5, 2e-5, 0.0])
    f8 = ctx.capsule_force(pos, prev)
    assert ctx.capsule_count() == 8 and f8.shape == (8, 6) and np.abs(f8[:, 2]).min() > 0
    g8 = ctx.capsule_grad(pos, prev, _dev(np.random.default_rng(1).normal(size=3 * s.tot_NV)))
    A8 = (a8, b8, ap8, bp8, np.full(8, R), np.full(8, 0.1), kn.full_mask(s.tot_NV, 8), s.k_capsule, s.eps_contact, s.eps_v * s.dt)
    g8_np = kn.capsule_grad(s.pos.to_numpy(), prev.cpu().numpy().reshape(-1, 3), np.random.default_rng(1).normal(size=(s.tot_NV, 3)), s.frozen.to_numpy().reshape(-1, 3), *A8)
    f8_np = kn.force(s.pos.to_numpy(), prev.cpu().numpy().reshape(-1, 3), *A8)
    assert g8.shape == (8, 14) and np.abs(g8_np).max() > 0
    for lo, hi in GRAD_GROUPS:
        assert np.abs(g8 - g8_np)[:, lo:hi].max() <= 1e-12 * np.abs(g8_np[:, lo:hi]).max(), (lo, hi)
    for lo, hi in FORCE_GROUPS:
        assert np.abs(f8 - f8_np)[:, lo:hi].max() <= 1e-12 * np.abs(f8_np[:, lo:hi]).max(), (lo, hi)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_rod import optimise
    losses, ends = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
    assert tuple(ends.shape) == (4, 1, 2, 3) and (ends[1:] != ends[0]).any()
