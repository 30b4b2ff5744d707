"""Sphere colliders (tsl_set_spheres; csrc/k_sphere.hpp) through the C ABI.  The reference has no such term: it is checked against
the dense NumPy restatement (tests/sphere_numpy.py), the half-space colliders in the limit of a large radius, and whole-rollout differences.  The
idiom is that of tests/test_gpu_colliders.py: a sphere quantity of a state is the difference against the same state with k_sphere = 0 -- no sphere
kernel runs there, and the rest is formed by the same launches in both -- and K = 2e5 N/m, the size of the cloth's own diagonal entries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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

    def part(self, fun, k=K, with_base=False):
        """fun() with k_sphere = k minus fun() with k_sphere = 0 (with_base: and the latter)"""
        self.ctx.set_param("k_sphere", k)
        a = fun()
        self.ctx.set_param("k_sphere", 0.0)
        b = fun()
        self.ctx.set_param("k_sphere", k)
        return (a - b, b) if with_base else a - b


def _drape(N, pin=True, perturb=0.0, newton_cap=200):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=DX * N, N=N, M=N, pin_row=pin, perturb=perturb, newton_cap=newton_cap)
    s.init_all()
    return s


RADII = np.array([1.0, 0.5])
MU = np.array([0.5, 0.3])


def pushed(x0, sel, eps, eh, seed):
    """the vertices `sel` of a flat horizontal sheet pushed partly through two balls of radius 1 m and 0.5 m under it whose tops lie in the sheet, both
    of them moving (c != cp, by about eps_v dt): distances and start-of-step distances to ball 0 on either side of the shell independently, slips
    relative to ball 0 of 0, 0.3 and 3 times eps_v dt; ball 1, its top a third of the sheet beside, meets whatever heights that gives.
    (centres, previous centres, x_prev, x)"""
    rng = np.random.default_rng(seed)
    x, xp = x0.copy(), x0.copy()
    mid = x0[sel].mean(axis=0)
    w = np.ptp(x0[sel, 0])
    c = np.array([[mid[0], mid[1], mid[2] - RADII[0]], [mid[0] + w / 3, mid[1], mid[2] - RADII[1] + 0.5 * eps]])
    cp = c - np.array([[0.4 * eh, 0.2 * eh, 0.6 * eh], [-0.2 * eh, 0.4 * eh, 0.2 * eh]])
    for v in sel:
        u0 = x0[v] - cp[0]; u0 /= np.linalg.norm(u0)
        xp[v] = cp[0] + (RADII[0] + rng.uniform(-0.5 * eps, 2.5 * eps)) * u0
        slip = rng.choice([0.0, 0.3 * eh, 3.0 * eh])
        a = rng.uniform(0, 2 * np.pi)
        t = np.array([np.cos(a), np.sin(a), 0.0]); t -= u0 * (u0 @ t); t /= np.linalg.norm(t)
        q = xp[v] + (c[0] - cp[0]) + slip * t - c[0]
        x[v] = c[0] + (RADII[0] + rng.uniform(-0.5 * eps, 2.5 * eps)) * q / np.linalg.norm(q)
    return c, cp, xp, x


def slips(x, xp, c, cp):
    return np.array([[sn.Pair(x[v], xp[v], c[j], cp[j], 1.0, 0.0, 1.0, 1.0, 1.0).r for j in range(len(c))] for v in range(len(x))])


def branches(x, xp, c, cp, R, mu, mask, eps, eh):
    """asserts that the state walks through every branch; returns the two active sets"""
    act, act0 = sn.active_sets(x, xp, c, cp, R, mask, eps)
    on = ((mask[:, None].astype(int) >> np.arange(len(c))) & 1).astype(bool)
    r = slips(x, xp, c, cp)
    fr = act0 & (mu[None, :] > 0)
    for a in (True, False):
        for b in (True, False):
            assert (on & (act == a) & (act0 == b)).any()
    assert (fr & (r < 1e-9)).any() and (fr & (r > 1e-9) & (r < eh)).any() and (fr & (r > eh)).any()
    assert (act.sum(axis=1) >= 2).any() and (fr.sum(axis=1) >= 2).any() and (mask == 0).any() and (on.sum(axis=1) == 1).any()
    assert np.abs(c - cp).min() > 0
    return act, act0


def _frozen_pattern(fz0, touched):
    """on top of the scene's own frozen dofs: all dofs of one touched vertex, one dof of a second, two of a third"""
    fz = fz0.copy()
    v0, v1, v2 = touched[:3]
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


def _check_state(S, x, xp, c, cp, mask, fz_list, eps, eh):
    """energy, gradient, operator in the spd modes 0, 1, 2 and with spd_literal, and the read-outs, of one state against the restatement.  Bound: 1e-12
    of the largest sphere entry, the colliders' bound."""
    ctx = S.ctx
    NV = len(x)
    args = (c, cp, RADII, MU, mask, K, eps, eh)
    assert ctx.sphere_count() == len(c)
    e_np, g_np = sn.energy(x, xp, *args), sn.gradient(x, xp, *args)
    H_ex, H_pr = sn.hessian(x, xp, *args, exact=True), sn.hessian(x, xp, *args, exact=False)
    B_np = sn.blocks(x, xp, *args)
    inside = np.zeros((3 * NV, 3 * NV), bool)
    for v in np.nonzero(np.abs(B_np).max(axis=(1, 2)) > 0)[0]:
        inside[3 * v:3 * v + 3, 3 * v:3 * v + 3] = True
    assert np.abs(H_ex - H_pr).max() > 1e-9 * np.abs(H_ex).max()          # (the curvature term is a million times over the bound)
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
            D, A = S.part(lambda spd=spd: S.operator(spd), with_base=True)
            ctx.set_param("spd_literal", 0)
            Hm = (H_ex if spd == 0 else H_pr) * ff
            print("%s: operator err / largest sphere entry %.2e, asymmetric entries of the difference / of the rest %d / %d"
                  % (tag, np.abs(D - Hm).max() / big, (D != D.T).sum(), (A != A.T).sum()))
            assert np.abs(D - Hm).max() <= 1e-12 * big
            assert (D[~inside] == 0).all() and (D[~free] == 0).all() and (D[:, ~free] == 0).all()
            assert not ((D != D.T) & (A == A.T)).any()
            got[tag] = (D, A)
        # spd 0 against spd 1: exactly the curvature term
        curv = (H_ex - H_pr) * ff
        dc = (got["spd 0"][0] - got["spd 1"][0]) - curv
        print("spd 0 - spd 1 against the curvature term: %.2e of the largest sphere entry (the term itself %.2e)" % (np.abs(dc).max() / big, np.abs(curv).max() / big))
        assert np.abs(dc).max() <= 1e-12 * big
        # the projected modes add the same numbers: the same bits wherever the rest of the operator has the same bits in both
        for tag in ("spd 2", "literal"):
            D1, A1 = got["spd 1"]; D2, A2 = got[tag]
            same = (A1 == A2) & inside
            print("%s against spd 1: %d of %d entries of the touched blocks lie on equal bits of the rest; largest difference %.2e of the largest sphere entry"
                  % (tag, same.sum(), inside.sum(), np.abs(D1 - D2).max() / big))
            assert (D1[same] == D2[same]).all() and np.abs(D1 - D2).max() <= 1e-12 * big
        # the read-outs (frozen dofs: not masked in the force, not counted in the gradients)
        fo, fo_np = ctx.sphere_force(S.pos, S.prev), sn.force(x, xp, *args)
        pn = np.random.default_rng(11).normal(size=(NV, 3))
        sg, sg_np = ctx.sphere_grad(S.pos, S.prev, _dev(pn.reshape(-1))), sn.sphere_grad(x, xp, pn, frozen, *args)
        print("force %.2e, sphere_grad %.2e of the largest entry" % (np.abs(fo - fo_np).max() / np.abs(fo_np).max(), np.abs(sg - sg_np).max() / np.abs(sg_np).max()))
        for lo, hi in ((0, 3), (3, 6), (6, 7), (7, 8)):
            print("  sphere_grad[:, %d:%d] %.2e of its largest entry" % (lo, hi, np.abs(sg - sg_np)[:, lo:hi].max() / np.abs(sg_np[:, lo:hi]).max()))
            assert np.abs(sg - sg_np)[:, lo:hi].max() <= 1e-12 * np.abs(sg_np[:, lo:hi]).max()
        assert np.abs(fo - fo_np).max() <= 1e-12 * np.abs(fo_np).max()
        assert np.abs(sg_np).min() > 0 and np.abs(fo_np[:, 2]).min() > 0


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("N", [8, 20])
def test_bare_cloth_matches_the_restatement(N):
    """N = 8: the 9 x 9-vertex cloth on the single-stream path; N = 20: 441 vertices, two workgroups with a partial one"""
    s = _drape(N)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    ctx.set_param("direct", 1)
    eps, eh = s.eps_contact, s.eps_v * s.dt
    NV = s.tot_NV
    assert NV == (N + 1) ** 2 and ctx.contact_counts() == (0, 0)
    c, cp, xp, x = pushed(s.pos.to_numpy(), np.arange(NV), eps, eh, seed=N)
    mask = sn.full_mask(NV, 2)
    mask[[3, 40]] = 0; mask[[5, 41, 50]] = 2; mask[[7, 60]] = 1
    act = branches(x, xp, c, cp, RADII, MU, mask, eps, eh)[0]
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    assert fz0.any()
    ctx.set_spheres(c, RADII, MU, mask)
    ctx.set_sphere_centres(c, cp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, x, xp, c, cp, mask, [fz0, _frozen_pattern(fz0, touched)], eps, eh)
    # new centres alone: the table follows; without previous centres the balls are at rest
    ctx.set_frozen(fz0.reshape(-1))
    c2 = c + [[1e-4, 0.0, -2e-4], [0.0, 1e-4, 1e-4]]
    for cpa, cpb in ((cp, cp), (None, c2)):
        ctx.set_sphere_centres(c2, cpa)
        e = S.part(S.energy)
        e_np = sn.energy(x, xp, c2, cpb, RADII, MU, mask, K, eps, eh)
        assert abs(e - e_np) <= 1e-12 * abs(e_np) and abs(e_np - sn.energy(x, xp, c, cp, RADII, MU, mask, K, eps, eh)) > 1e-3 * abs(e_np)
    s._close_ctx()


def test_cloth_with_the_ball_matches_the_restatement():
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
    c, cp, xp, x = pushed(x0, cloth, eps, eh, seed=5)
    mask = np.zeros(NV, np.uint8)          # (the bodies see no sphere)
    mask[cloth] = 3; mask[cloth[[3, 40]]] = 0; mask[cloth[[5, 41, 50]]] = 2; mask[cloth[[7, 60]]] = 1
    act = branches(x, xp, c, cp, RADII, MU, mask, eps, eh)[0]
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_spheres(c, RADII, MU, mask)
    ctx.set_sphere_centres(c, cp)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [v for v in np.nonzero(act.any(axis=1))[0] if not fz0[v].any()]
    _check_state(S, x, xp, c, cp, mask, [fz0, _frozen_pattern(fz0, touched)], eps, eh)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ all classes at once
def test_handles_ties_planes_and_a_ball_in_one_scene():
    """Scene_seam (two 8 x 8 cloths, nine ties) with vertex handles, two planes and two balls: the energy of all four equals the sum of the
    restatements (the partials of every class lie where energy_async says), and the handle, tie and plane numbers keep their bits with spheres on"""
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
    c, cp, xp, x = pushed(x0, np.arange(NV), eps, eh, seed=9)
    n = cn.unit([[0.0, 0.0, 1.0], [0.0, np.sin(0.3), np.cos(0.3)]])
    o = np.array([float(x0[:, 2].mean()), float(n[1] @ x0.mean(axis=0)) + 0.5 * eps])
    mu_p = np.array([0.5, 0.3])
    pmask = cn.full_mask(NV, 2); pmask[::7] = 1; pmask[3] = 0
    smask = sn.full_mask(NV, 2); smask[::5] = 2; smask[4] = 0
    idx, b, w = tn.records(s.faces.to_numpy(), s._tie_v, s._tie_f, s._tie_b)
    S = _State(ctx, x, xp, s._ref_angle)
    fz = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_colliders(n, o, mu_p, pmask); ctx.set_param("k_collider", K)

    def numbers():
        p = _dev(np.random.default_rng(4).normal(size=3 * NV))
        return (ctx.handle_force(S.pos), ctx.handle_grad(p), ctx.tie_force(S.pos), ctx.tie_grad(S.pos, p), ctx.contact_blocks(False),
                ctx.collider_force(S.pos, S.prev), ctx.collider_grad(S.pos, S.prev, p), ctx.param_grads(S.pos, S.ref, ["k_handle", "k_tie"], p=p))
    S.operator(1)
    before = numbers()
    e_htc, g_htc = S.energy(), S.grad()
    ctx.set_param("k_handle", 0.0); ctx.set_param("k_tie", 0.0); ctx.set_param("k_collider", 0.0)
    e_0 = S.energy()
    ctx.set_param("k_handle", K); ctx.set_param("k_tie", K); ctx.set_param("k_collider", K)
    ctx.set_spheres(c, RADII, MU, smask); ctx.set_sphere_centres(c, cp); ctx.set_param("k_sphere", K)
    S.operator(1)
    after = numbers()
    for a, d in zip(before[:7], after[:7]):
        assert np.array_equal(a, d)
    assert before[7] == after[7] and ctx.tie_count() == 9 and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 9
    e_all, g_all = S.energy(), S.grad()
    e_h, e_t, e_c = hn.energy(x, hv, hw, ht, K), tn.energy(x, idx, b, w, K), cn.energy(x, xp, n, o, mu_p, pmask, K, eps, eh)
    e_s = sn.energy(x, xp, c, cp, RADII, MU, smask, K, eps, eh)
    print("energy of the four classes %.17g, restatements %.17g + %.17g + %.17g + %.17g" % (e_all - e_0, e_h, e_t, e_c, e_s))
    tot = e_h + e_t + e_c + e_s
    assert min(e_h, e_t, e_c, e_s) > 1e-6 * tot          # (a class whose partials were lost or read twice would show a million times over the bound)
    assert abs((e_all - e_0) - (((e_h + e_t) + e_c) + e_s)) <= 1e-12 * tot
    assert abs((e_all - e_htc) - e_s) <= 1e-12 * tot
    gs = sn.gradient(x, xp, c, cp, RADII, MU, smask, K, eps, eh) * (fz == 0)
    assert np.abs((g_all - g_htc) - gs).max() <= 1e-12 * max(np.abs(gs).max(), np.abs(g_all).max())
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
    used.set_spheres([[mid[0], mid[1], -0.05 - 1e-4], [mid[0] + 0.02, mid[1], -0.02]], [0.05, 0.02], [0.5, 0.2], 2000.0)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    used.set_sphere_centres(used._sph_c + [1e-5, 0.0, 1e-5])
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and ctx_u.sphere_count() == 2 and np.abs(used.sphere_force()).max() > 0
    assert not np.array_equal(_assemble_and_step(ctx_u, y, used._ref_angle)[0], want[0])
    if how == "removed":
        used.set_spheres([], [], [], 0.0)
        assert used._ensure_ctx() is ctx_u and ctx_u.sphere_count() == 0
    else:
        ctx_u.set_param("k_sphere", 0.0)
        f = ctx_u.sphere_force(_dev(y), _dev(y))
        assert ctx_u.sphere_count() == 2 and f.shape == (2, 3) and not f.any()
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, c in zip(want, got):
        assert np.array_equal(a, c)
    fresh._close_ctx(); used._close_ctx()


# ------------------------------------------------------------------------------------------------ the large-radius limit is the half-space
def _floor(**kw):
    from thinshelllab_amd.task_scene.Scene_floor import Scene
    s = Scene(N=8, **kw)
    s.init_all()
    s._ensure_ctx().set_param("direct", 1)
    return s


BIG_R = 1.0e4
REST_BOUND = 4e-7     # relative: the bound of test_resting_depth_is_m_g_over_k (tests/test_gpu_colliders.py)


def _on_big_ball(mu=0.5, **kw):
    """Scene_floor with its plane taken away and a ball of radius 1e4 m in its place whose top is the plane"""
    s = _floor(mu=mu, **kw)
    k = s.k_collider
    s.set_colliders([], [], [], 0.0)
    s.set_spheres([[0.0, 0.0, -BIG_R]], [BIG_R], [mu], k)
    return s


def _depth_on_ball(x, c):
    """d of every vertex to the big ball, in extended precision (|q| ~ 1e4 m: a double's last bit there is 2e-12 m)"""
    q = x.astype(np.longdouble) - np.asarray(c, np.longdouble)
    return (np.sqrt((q * q).sum(axis=1)) - np.longdouble(BIG_R)).astype(np.float64)


def test_a_large_ball_is_the_half_space():
    """Scene_floor's resting case (a cloth set down on the shell's surface, 16 steps) on its plane and on a ball of R = 1e4 m whose top is the plane.
    The two distances of a point of the sheet differ by at most s^2 / (2 R) = 4e-8 m (s = 0.028 m, the half diagonal); the final positions agree within
    ten times that (the margin is for the dynamics); the mean depth is m g / k and the ball carries the weight within the colliders' bound."""
    k = 2e3
    runs = {}
    for tag, make in (("plane", lambda: _floor(k_collider=k, depth=0.0)), ("ball", lambda: _on_big_ball(k_collider=k, depth=0.0))):
        s = make()
        for f in range(1, 17):
            st = s.time_step(None, f)
            assert st["unconverged"] == 0 and st["factorizations"] > 0, st
        runs[tag] = (s.pos.to_numpy().copy(), s.collider_force() if tag == "plane" else s.sphere_force(), s.cloths[0].mass, s.eps_contact, s.tot_NV)
        assert (s.n_collider, s.n_sphere) == ((1, 0) if tag == "plane" else (0, 1))
        s._close_ctx()
    xb, fb, m, eps, NV = runs["ball"]
    xpl = runs["plane"][0]
    geo = 0.5 * (0.02 ** 2 + 0.02 ** 2) / BIG_R
    d_s, d_p = _depth_on_ball(xb, [0.0, 0.0, -BIG_R]), xb[:, 2]
    print("|d_sphere - d_plane| over the sheet: %.3e m (s^2 / 2R = %.3e m); final positions of the two runs differ by %.3e m" % (np.abs(d_s - d_p).max(), geo, np.abs(xb - xpl).max()))
    assert abs(geo - 4e-8) < 1e-12 and np.abs(d_s - d_p).max() <= geo * (1 + 1e-6)
    assert np.abs(xb - xpl).max() <= 10 * geo
    depth = float((eps - d_s).mean())
    print("ball: mean depth %.9e m, m g / k %.9e m, deviation %.2e relative; force %s N, weight %.9e N" % (depth, m * 9.8 / k, abs(depth - m * 9.8 / k) / (m * 9.8 / k), fb, m * 9.8 * NV))
    assert (d_s < eps).all() and abs(depth - m * 9.8 / k) <= REST_BOUND * (m * 9.8 / k)
    assert abs(fb[0, 2] - m * 9.8 * NV) <= 10 * REST_BOUND * m * 9.8 * NV and np.abs(fb[0, :2]).max() <= 1e-6 * m * 9.8 * NV


def test_a_ball_that_moves_sideways_drags_the_sheet():
    """the same ball, 12 steps, its centre moving along +x by eps_v dt per step: with mu = 0.5 the sheet follows, with mu = 0 it does not (the normals'
    x components, |x| / R <= 2e-6, cancel over the symmetric sheet up to the ball's own shift: g v t^3 / (6 R) = 3.5e-10 m)"""
    moved = {}
    for mu in (0.5, 0.0):
        s = _on_big_ball(mu=mu, k_collider=2e3)
        x0 = s.pos.to_numpy()
        step = s.eps_v * s.dt
        for f in range(1, 13):
            s.set_sphere_centres([[step * f, 0.0, -BIG_R]])
            assert s.time_step(None, f)["unconverged"] == 0
        moved[mu] = float((s.pos.to_numpy() - x0)[:, 0].mean())
        print("mu %.1f: mean x displacement %.6e m, the ball moved %.6e m: dragged fraction %.4f" % (mu, moved[mu], 12 * step, moved[mu] / (12 * step)))
        s._close_ctx()
    assert moved[0.5] > 0 and moved[0.5] > moved[0.0] and abs(moved[0.0]) < 1e-9


# ------------------------------------------------------------------------------------------------ whole rollouts
STVK = (3.0e5, 2.0e5)
BALL_R, BALL_PUSH, BALL_K = 0.04, 1.5e-3, 2.0e3


def _ball(N=8, **kw):
    from thinshelllab_amd.task_scene.Scene_ball import Scene
    s = Scene(N=N, radius=BALL_R, push=BALL_PUSH, k_sphere=BALL_K, **kw)
    s.init_all()
    s._ensure_ctx().set_param("direct", 1)
    return s


_RELAXED = {}


def _relaxed():
    """the rollout scene's start, computed once: the StVK sheet without bending (its matrix is the exact second derivative of its energy, as the sheet
    of DESIGN.md 2.4), corners frozen, pushed up in the middle by a ball of radius 4 cm (the sheet's side) whose top lies 1.5 mm above the corners'
    plane, after 40 steps (positions, velocities)"""
    if not _RELAXED:
        s = _ball(Kb=0.0, stvk=STVK)
        for f in range(1, 41):
            assert s.time_step(None, f)["unconverged"] == 0
        _RELAXED["x"], _RELAXED["v"] = s.pos.to_numpy().copy(), s.vel.to_numpy().copy()
        s._close_ctx()
    return _RELAXED["x"].copy(), _RELAXED["v"].copy()


def _ball_trajectory(T, c0, eh):
    """the ball moves up and sideways: sideways steps of 0.4, 1.6 and 2.8 eps_v dt, so that the slip per step straddles eps_v dt"""
    c = np.tile(c0, (T, 1, 1))
    for f in range(1, T):
        c[f, 0] = c[f - 1, 0] + [(0.4 + 1.2 * (f - 1)) * eh, 0.3 * eh, 2e-6]
    return c


# The two difference steps of every check, a decade apart, as fractions of the parameter's own scale: centres and start positions against the slip
# scale eps_v dt = 5e-5 m (2 % and 0.2 %), the radius against the shell eps = 4e-4 m (2.5 % and 0.25 %), mu against mu = 0.5 (20 % and 2 %).  The
# differences are those of the time stepper as it is: its Newton iteration stops at |p|max / dt < 1e-7 and converges linearly on this scene
# (about 0.3 per iteration), so they differentiate an iterate 1e-6 .. 5e-5 relative away from the stationary point that the reverse step assumes.
# Steps this size keep the differences' own disagreement above that; DESIGN.md 2.9 has the differences at every step from 1e-5 to 1e-8.
FD_STEPS = {"c": (1e-6, 1e-7), "mu": (1e-1, 1e-2), "R": (1e-5, 1e-6), "x": (1e-6, 1e-7)}


def _rollout_checks(steps=FD_STEPS):
    """the rollout of test_whole_rollout_gradients_match_differences: ([(name, analytic, (difference at the larger step, at the smaller step))],
    smallest and largest slip of an active pair in one step of the tape in units of eps_v dt, number of active vertices)"""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    x0, v0 = _relaxed()
    s = _ball(Kb=0.0, stvk=STVK)
    NV = s.tot_NV
    eps, eh = s.eps_contact, s.eps_v * s.dt
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)
    c0, R0, mu0 = s.ball()
    c_traj = _ball_trajectory(T, c0, eh)
    mask = s._sph_mask.copy()
    free = (s.frozen.to_numpy().reshape(-1, 3) == 0)
    sets = []

    def rollout(c=c_traj, mu=mu0, R=R0, x=x0, reverse=False):
        s.set_spheres(c[0], R, mu, BALL_K)
        # (row 0 of the tape is d(loss)/d(x_0) with the state before it held fixed: the start velocity moves with the start state)
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.from_numpy(v0 + (x - x0) * (s.damping / s.dt))
        g = Grad(s, T, 0); g.init_mass(s)
        g.count_kb_grad = False
        g.copy_pos(s, 0)
        for fr in range(1, T):
            s.set_sphere_centres(c[fr])
            st = s.time_step(None, fr)
            assert st["unconverged"] == 0 and st["newton_iters"] < 50
            if reverse:
                print("step %d: %d Newton iterations, last delta %.2e" % (fr, st["newton_iters"], st["last_delta"]))
            g.copy_pos(s, fr)
        xs = g.pos_buffer.t.cpu().numpy()
        sets.append([sn.active_sets(xs[fr], xs[fr - 1], c[fr], c[fr - 1], R, mask, eps) for fr in range(1, T)])
        L = float((xs[T - 1] * wgt).sum())
        if not reverse:
            return L
        assert np.array_equal(g.sphere_centres.t.numpy(), c) and np.array_equal(g.sphere_centres_prev.t.numpy()[1:], c[:-1])
        g.pos_grad.t[T - 1] = _dev(wgt)
        for fr in range(T - 1, 0, -1):
            g.transfer_grad(fr, s, None)
            assert g.last_stats["flag"] != 3 and g.pos_grad.t[fr - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.sphere_grad.t.numpy().copy(), g.sphere_centre_grad().numpy().copy(), g.pos_grad.t[0].cpu().numpy().copy(), xs

    _, sg, cg, pg0, xs = rollout(reverse=True)
    assert sg.shape == (T, 1, 8) and cg.shape == (T, 1, 3) and (sg[0] == 0).all() and np.abs(sg[1:]).min() > 0
    assert np.array_equal(cg[:-1], sg[:-1, :, 0:3] + sg[1:, :, 3:6])
    slip = np.array([slips(xs[fr], xs[fr - 1], c_traj[fr], c_traj[fr - 1])[:, 0] for fr in range(1, T)])
    act = np.array([a[0][:, 0] & a[1][:, 0] for a in sets[0]])
    n_act = int(act.all(axis=0).sum())
    print("active vertices per step %s, on every step %d; slip per step of the active pairs: %.3e .. %.3e m, eps_v dt = %.1e m"
          % (act.sum(axis=1), n_act, slip[act].min(), slip[act].max(), eh))
    d_c = rng.uniform(-1.0, 1.0, (T, 1, 3))
    d_mu = rng.uniform(0.5, 1.0, 1)
    d_R = rng.uniform(0.5, 1.0, 1)
    e = rng.normal(size=x0.shape) * free
    fd = lambda f, hs: [(f(h) - f(-h)) / (2 * h) for h in hs]
    checks = [("sphere_centre_grad . delta_c", float((cg * d_c).sum()), fd(lambda h: rollout(c=c_traj + h * d_c), steps["c"])),
              ("sphere_grad[:, :, 6] . delta_mu", float((sg[:, :, 6].sum(axis=0) * d_mu).sum()), fd(lambda h: rollout(mu=mu0 + h * d_mu), steps["mu"])),
              ("sphere_grad[:, :, 7] . delta_R", float((sg[:, :, 7].sum(axis=0) * d_R).sum()), fd(lambda h: rollout(R=R0 + h * d_R), steps["R"])),
              ("pos_grad[0] . direction", float((pg0 * e).sum()), fd(lambda h: rollout(x=x0 + h * e), steps["x"]))]
    for i, a in enumerate(sets[1:]):
        for fr in range(T - 1):
            assert np.array_equal(a[fr][0], sets[0][fr][0]) and np.array_equal(a[fr][1], sets[0][fr][1]), "a vertex crossed the shell between the runs: a badly chosen input (perturbed run %d)" % i
    for name, got, d in checks:
        print("%s: analytic %.10e, differences %s" % (name, got, " / ".join("%.10e" % v for v in d)))
        print("    (the last two disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (abs(d[-2] - d[-1]) / abs(d[-1]), abs(got - d[-1]) / abs(d[-1]), 3 * abs(d[-2] - d[-1]) / abs(d[-1])))
    s._close_ctx()
    return checks, (slip[act].min() / eh, slip[act].max() / eh), n_act


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last state; Scene_ball with the
    StVK sheet without bending, relaxed over the ball for 40 steps; the ball then moves up by 2e-6 m and sideways by 0.4, 1.6 and 2.8 eps_v dt per
    step.  sphere_centre_grad() contracted with a random trajectory direction, the mu and R columns summed over the steps, and pos_grad[0] . e along
    a random free direction (the state before it held fixed), each against central differences at two steps a decade apart.  Bound: three times the
    disagreement of the two differences, which must itself be below 1e-2 of the value.  No vertex may cross d = eps or d0 = eps between the runs.
    Measured at FD_STEPS: errors 5.6e-5, 2.6e-6, 5.6e-7 and 4.1e-5 relative against bounds of 1.1e-3, 9.3e-5, 1.8e-5 and 1.0e-4; five active vertices,
    slips of 0.46 .. 2.8 eps_v dt.  At finer steps the differences agree with each other to 1e-6 .. 1e-8 while their distance to the analytic values
    stays at 5e-5, 2.9e-6, 6.3e-7 and 4.0e-5: the rule would miss there, see FD_STEPS and DESIGN.md 2.9."""
    checks, (slip_min, slip_max), n_act = _rollout_checks()
    assert slip_max > 1.0 > slip_min > 2e-5          # both friction regimes on the tape (in units of eps_v dt; 2e-5: the r > 1e-9 switch of the block)
    assert n_act >= 5
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


def _moving(shift):
    s = _ball()
    c0 = s.ball()[0]
    return s, (lambda f: c0 + np.asarray(shift) * f)


def test_group_members_equal_their_single_runs_and_two_runs_repeat():
    from thinshelllab_amd.scene_group import SceneGroup
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(81, 3))
    A, B = (2e-5, 1e-5, 2e-6), (-4e-5, 0.0, -1e-6)
    runs = {}
    for tag, shift in (("a", A), ("b", A), ("c", B)):
        s, c_of = _moving(shift)
        g = _tape(s)
        for f in range(1, T_TAPE):
            s.set_sphere_centres(c_of(f))
            st = s.time_step(None, f)
            assert st["unconverged"] == 0 and st["factorizations"] > 0, st
            g.copy_pos(s, f)
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
        for f in range(T_TAPE - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.last_stats["flag"] != 3
        runs[tag] = (g.pos_buffer.t.cpu().numpy().copy(), g.pos_grad.t.cpu().numpy().copy(), g.sphere_grad.t.numpy().copy(), g.sphere_centres.t.numpy().copy())
        s._close_ctx()
    for a, b in zip(runs["a"], runs["b"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(runs["a"][0], runs["c"][0]) and np.abs(runs["a"][2][1:, :, :6]).min() > 0 and (runs["a"][2][0] == 0).all()
    members = [_moving(A), _moving(B)]
    ms = [m[0] for m in members]
    G = SceneGroup(ms)
    gs = [_tape(m) for m in ms]
    for f in range(1, T_TAPE):
        for m, c_of in members:
            m.set_sphere_centres(c_of(f))
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
        assert np.array_equal(gs[i].sphere_grad.t.numpy(), runs[tag][2]) and np.array_equal(gs[i].sphere_centres.t.numpy(), runs[tag][3]), i
        assert np.array_equal(gs[i].sphere_centres_prev.t.numpy()[1:], runs[tag][3][:-1])
    for m in ms:
        m._close_ctx()


def test_spheres_build_no_plan_and_no_slot():
    """the factorised path: the plan count after the first step does not change when spheres are switched on, over the rollout or in the reverse sweep"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    T = 4
    s = _ball()
    centre, radius, mu = s.ball()
    s.set_spheres([], [], [], 0.0)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    st = s.time_step(None, 1)
    assert st["unconverged"] == 0 and st["factorizations"] > 0 and ctx.sphere_count() == 0
    plans = ctx.direct_info()["plans"]
    assert plans >= 1
    s.set_spheres(centre, radius, mu, BALL_K)
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    for f in range(1, T):
        s.set_sphere_centres(centre + [[1e-5 * f, 0.0, 0.0]])
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0 and st["nc"] == 0, st
        g.copy_pos(s, f)
        assert ctx.direct_info()["plans"] == plans and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 0
    assert s._ensure_ctx() is ctx and ctx.sphere_count() == 1 and np.abs(s.sphere_force()).max() > 0
    g.pos_grad.t[T - 1] = _dev(np.random.default_rng(7).normal(scale=1e-2, size=(s.tot_NV, 3)))
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3
    assert ctx.direct_info()["plans"] == plans and np.abs(g.sphere_grad.t.numpy()[1:]).max() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_keep_the_previous_list():
    s = _ball()
    ctx = s._ensure_ctx()
    c0, R0, mu0 = s.ball()
    ctx.set_spheres(np.vstack([c0, c0 + [0.0, 0.01, 0.0]]), [BALL_R, BALL_R], [0.5, 0.1])
    pos = _dev(s.pos.to_numpy())
    before = ctx.sphere_force(pos, pos)
    assert before.shape == (2, 3) and np.abs(before).max() > 0
    o = [0.0, 0.0, -1.0]
    cases = [(([o, [0.0, np.nan, 0.0]], [1.0, 1.0], [0.1, 0.1]), r"centre \(0, nan, 0\) of sphere 1 is not finite"),
             (([o, o], [1.0, 0.0], [0.1, 0.1]), r"radius 0 of sphere 1 is not finite and positive"),
             (([o, o], [1.0, np.inf], [0.1, 0.1]), r"radius inf of sphere 1 is not finite and positive"),
             (([o, o], [1.0, 1.0], [0.1, -0.5]), r"friction coefficient -0.5 of sphere 1 is negative or not finite"),
             (([o] * 9, [1.0] * 9, [0.1] * 9), r"9 spheres: at most 8")]
    for args, pat in cases:
        with pytest.raises(Exception, match="tsl_set_spheres: " + pat):
            ctx.set_spheres(*args)
        with pytest.raises(ValueError, match="set_spheres: " + pat):          # the scene's host check: the library's message
            s.set_spheres(*args, 10.0)
        assert ctx.sphere_count() == 2 and np.array_equal(ctx.sphere_force(pos, pos), before)
    bad = np.full(s.tot_NV, 3, np.uint8); bad[17] = 4
    with pytest.raises(Exception, match=r"tsl_set_spheres: mask 0x04 of vertex 17 names a sphere at or above 2"):
        ctx.set_spheres([o, o], [1.0, 1.0], [0.1, 0.1], bad)
    with pytest.raises(Exception, match=r"tsl_set_sphere_centres: centre \(inf, 0, -1\) of sphere 0 is not finite"):
        ctx.set_sphere_centres([[np.inf, 0.0, -1.0], o])
    with pytest.raises(Exception, match=r"tsl_set_sphere_centres: previous centre \(0, 0, nan\) of sphere 1 is not finite"):
        ctx.set_sphere_centres([o, o], [o, [0.0, 0.0, np.nan]])
    assert ctx.sphere_count() == 2 and np.array_equal(ctx.sphere_force(pos, pos), before)
    with pytest.raises(Exception, match="k_sphere must be finite and >= 0"):
        ctx.set_param("k_sphere", -1.0)
    with pytest.raises(Exception, match="k_sphere must be finite and >= 0"):
        ctx.set_param("k_sphere", np.nan)
    # eight are the most: accepted, and the list is the new one
    c8 = c0 + np.arange(8)[:, None] * [0.0, 0.002, 0.0]
    ctx.set_spheres(c8, [BALL_R] * 8, [0.1] * 8)
    f8 = ctx.sphere_force(pos, pos)
    assert ctx.sphere_count() == 8 and f8.shape == (8, 3) and np.array_equal(f8[0], before[0]) and np.abs(f8[:, 2]).min() > 0
    g8 = ctx.sphere_grad(pos, pos, _dev(np.random.default_rng(1).normal(size=3 * s.tot_NV)))
    g8_np = sn.sphere_grad(s.pos.to_numpy(), s.pos.to_numpy(), np.random.default_rng(1).normal(size=(s.tot_NV, 3)), s.frozen.to_numpy().reshape(-1, 3), c8, c8,
                           np.full(8, BALL_R), np.full(8, 0.1), sn.full_mask(s.tot_NV, 8), BALL_K, s.eps_contact, s.eps_v * s.dt)
    assert g8.shape == (8, 8) and np.abs(g8 - g8_np).max() <= 1e-12 * np.abs(g8_np).max()
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_ball import optimise
    losses, centres = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
    assert tuple(centres.shape) == (4, 1, 3) and (centres[1:] != centres[0]).any()
