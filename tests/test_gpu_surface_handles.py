"""Soft handles at barycentric points of faces (tsl_set_handles_on_faces; csrc/k_handle.hpp) through the C ABI.  The reference has
no such term: it is checked against the dense NumPy restatement (tests/surface_handle_numpy.py), the vertex handles, differences of the assembled
gradient and whole-rollout differences.  The idiom is that of tests/test_gpu_handles.py: a handle quantity of a state is the difference against the
same state with k_handle = 0 -- no handle kernel runs there and the rest is formed by the same launches in both -- and K = 2e5 N/m, the size of
the cloth's own diagonal entries, so that a difference of two assembled matrices still holds the handle term to the digits asked for."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_numpy as fn  # noqa: E402
import surface_handle_numpy as sn  # noqa: E402

pytestmark = pytest.mark.gpu

K = 2.0e5


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _cloth(N, pin=False, perturb=0.0, Kb=100.0, newton_cap=200, stvk=None):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=0.1 / 15 * N, N=N, M=N, Kb=Kb, pin_row=pin, perturb=perturb, newton_cap=newton_cap)
    if stvk:
        c = s.cloths[0]
        c.stvk_mu[None], c.stvk_lam[None] = stvk
        c.membrane[None] = 1.0
    s.init_all()
    return s


class _State:
    """one state of a context: positions, zero velocity, rest angles; energy / gradient / matrix of it as NumPy"""

    def __init__(self, s, x):
        self.ctx = s._ensure_ctx()
        self.pos = _dev(x); self.prev = self.pos.clone(); self.vel = torch.zeros_like(self.pos)
        self.ref = s._ref_angle

    def energy(self):
        return self.ctx.energy(self.pos, self.prev, self.vel, self.ref)

    def grad(self, spd=0):
        F = torch.zeros(self.pos.numel(), dtype=torch.float64, device="cuda")
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd, grad=F)
        return F.cpu().numpy().reshape(-1, 3)

    def matrix(self, spd):
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd)
        return self.ctx.matrix_csr().toarray()

    def handle_part(self, fun, k=K, with_base=False):
        """fun() with k_handle = k minus fun() with k_handle = 0 (with_base: and the latter)"""
        self.ctx.set_param("k_handle", k)
        a = fun()
        self.ctx.set_param("k_handle", 0.0)
        b = fun()
        self.ctx.set_param("k_handle", k)
        return (a - b, b) if with_base else a - b


def _sparse_lists(tab):
    """seven handles: an interior point, a point on an edge, a (1, 0, 0) point, two on one face, two of different faces that meet in a vertex; one weight 0"""
    f1 = 120
    f2 = next(f for f in range(len(tab)) if f != f1 and tab[f1][0] in tab[f] and len(set(tab[f]) & set(tab[f1])) == 1)
    f = np.array([100, 50, 7, 200, 200, f1, f2], np.int32)
    b = np.array([[0.2, 0.5, 0.3], [0.0, 0.4, 0.6], [1.0, 0.0, 0.0], [0.6, 0.3, 0.1], [0.1, 0.1, 0.8], [0.5, 0.25, 0.25], [0.3, 0.3, 0.4]])
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 0.75, 1.25])
    return f, b, w


def _case(name):
    """(scene, x, faces, fv, b, w, t): the perturbed gravity-free drape cloth at N = 12 (169 vertices, 288 faces) with face handles.  'dense': three on
    every face in shuffled order, 864 in all -- four energy workgroups with a partial wave, up to 24 entries per vertex, every face block touched"""
    s = _cloth(12)
    s._ensure_ctx().set_gravity(np.zeros((s.tot_NV, 3)))
    rng = np.random.default_rng({"dense": 31, "sparse": 32}[name])
    dx = s.cloths[0].dx
    x = s.pos.to_numpy() + rng.normal(scale=0.15 * dx, size=(s.tot_NV, 3))
    tab = s.faces.to_numpy()
    assert tab.shape == (288, 3) and s.tot_NV == 169
    if name == "dense":
        f = rng.permutation(np.repeat(np.arange(288), 3)).astype(np.int32)
        b = rng.dirichlet(np.ones(3), len(f))
        w = rng.uniform(0.25, 2.0, len(f))
    else:
        f, b, w = _sparse_lists(tab)
    fv = tab[f]
    t = sn.points(x, fv, b) + rng.normal(scale=0.5 * dx, size=(len(f), 3))
    s.set_surface_handles(f, b, K, w)
    s.set_handle_targets(t)
    return s, x, f, fv, b, w, t


def _frozen_pattern(NV, fv):
    """all dofs of one touched vertex, one dof of a second, two of a third"""
    fz = np.zeros((NV, 3), np.int32)
    v0, v1, v2 = fv[2, 0], fv[0, 1], fv[1, 2]
    assert len({int(v0), int(v1), int(v2)}) == 3
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


# ------------------------------------------------------------------------------------------------ per state
def _check_state(S, x, fv, b, w, t, frozen, rest_is_exact):
    """the per-state checks against the restatement at the state S (its context holds the face handles with k_handle = K).  rest_is_exact: the cloth's
    stiffnesses are zero, only the mass diagonal shares entries with the handles, so the rest cancels bit for bit and the three spd modes must give
    the same bits; with element blocks in place each mode is held to the restatement within the bound.
    Symmetry: blocks (v_a, v_b) and (v_b, v_a) receive the same sum s, so the difference fl(A + s) - A equals its transpose bit for bit wherever the
    rest of the matrix A does.  The cloth's own assembled blocks are symmetric only to the last bits in some entries (the count is printed; the mass
    diagonal alone is symmetric); the roundings of fl(A_ab + s) and fl(A_ba + s) may differ there, so an entry of the difference may differ from its
    mirror image only where A does."""
    NV = len(x)
    fzb = frozen.astype(bool)
    e = S.handle_part(S.energy)
    e_np = sn.energy(x, fv, b, w, t, K)
    print("energy %.17g restatement %.17g rel %.2e" % (e, e_np, abs(e - e_np) / abs(e_np)))
    assert abs(e - e_np) <= 1e-12 * abs(e_np)
    g = S.handle_part(S.grad)
    g_np = sn.gradient(x, fv, b, w, t, K, frozen)
    print("gradient err / max %.2e" % (np.abs(g - g_np).max() / np.abs(g_np).max()))
    assert np.abs(g - g_np).max() <= 1e-12 * np.abs(g_np).max()
    assert (g[fzb] == 0).all()
    DB = [S.handle_part(lambda spd=spd: S.matrix(spd), with_base=True) for spd in (0, 1, 2)]
    D, base = [d for d, _ in DB], [a for _, a in DB]
    H = sn.matrix(NV, fv, b, w, K, frozen)
    inside = sn.touched(NV, fv)
    print("matrix: err / largest handle entry %.2e, outside the touched blocks max %.2e, asymmetric entries of the difference / of the rest of the matrix at spd 0, 1, 2: %s, entries where spd 1 / spd 2 differ from spd 0: %d / %d"
          % (np.abs(D[0] - H).max() / np.abs(H).max(), np.abs(D[0][~inside]).max(),
             ", ".join("%d / %d" % ((d != d.T).sum(), (a != a.T).sum()) for d, a in DB), (D[1] != D[0]).sum(), (D[2] != D[0]).sum()))
    if rest_is_exact:
        assert np.array_equal(D[0], D[1]) and np.array_equal(D[0], D[2])
    if rest_is_exact:
        assert all(np.array_equal(a, a.T) for a in base)      # (so the differences are held to bit symmetry in every entry)
    for Dm, A in DB:
        assert np.abs(Dm - H).max() <= 1e-12 * np.abs(H).max()
        assert (Dm[~inside] == 0).all()
        assert (Dm[fzb.ravel()] == 0).all() and (Dm[:, fzb.ravel()] == 0).all()
        assert not ((Dm != Dm.T) & (A == A.T)).any()


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_energy_gradient_and_matrix_match_the_restatement(name):
    s, x, f, fv, b, w, t = _case(name)
    S = _State(s, x)
    NV = s.tot_NV
    free, fz = np.zeros((NV, 3), np.int32), _frozen_pattern(NV, fv)
    for exact in (False, True):   # the cloth as it is, then with its stiffnesses at zero: only the mass diagonal under the handle entries
        if exact:
            for k in ("Kl", "Ka", "Kb"):
                S.ctx.set_param("cloth0." + k, 0.0)
        for frozen in (free, fz):
            S.ctx.set_frozen(frozen.reshape(-1))
            _check_state(S, x, fv, b, w, t, frozen, exact)
    s._close_ctx()


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_read_outs_and_stiffness_key(name):
    s, x, f, fv, b, w, t = _case(name)
    S = _State(s, x)
    ctx, NV = S.ctx, s.tot_NV
    fz = _frozen_pattern(NV, fv)
    ctx.set_frozen(fz.reshape(-1))
    assert np.array_equal(ctx.handle_targets(), t)
    pts, pts_np = ctx.handle_points(S.pos), sn.points(x, fv, b)
    assert np.abs(pts - pts_np).max() <= 1e-14 * np.abs(pts_np).max()
    fo, fo_np = ctx.handle_force(S.pos), sn.force(x, fv, b, w, t, K)
    assert np.abs(fo - fo_np).max() <= 1e-14 * np.abs(fo_np).max()
    pn = np.random.default_rng(11).normal(size=3 * NV)
    p = _dev(pn)
    tg, tg_np = ctx.handle_grad(p), sn.target_grad(pn, fv, b, w, K, fz)
    print("points %.2e, force %.2e, handle_grad %.2e of the largest entry" % (np.abs(pts - pts_np).max() / np.abs(pts_np).max(),
          np.abs(fo - fo_np).max() / np.abs(fo_np).max(), np.abs(tg - tg_np).max() / np.abs(tg_np).max()))
    assert np.abs(tg - tg_np).max() <= 1e-14 * np.abs(tg_np).max()
    # exact zeros where every contributing dof is frozen (or carries no weight); the force read-out is not masked
    dead = (np.einsum("ia,iac->ic", (b > 0).astype(float), 1.0 - fz[fv]) == 0) | (w == 0)[:, None]
    assert (tg[dead] == 0).all() and (tg[~dead] != 0).all() and (dead.any() or name == "dense")
    if name == "sparse":
        assert (tg[2] == 0).all() and (fo[2] != 0).all()     # the (1, 0, 0) handle sits on the vertex with all dofs frozen
    # the k_handle key against central differences of the assembled (masked) gradient: the term is linear in k_handle
    got = ctx.param_grads(S.pos, S.ref, ["k_handle"], p=p)["k_handle"]
    h = 0.5 * K
    ctx.set_param("k_handle", K + h); gp = S.grad()
    ctx.set_param("k_handle", K - h); gm = S.grad()
    ctx.set_param("k_handle", K)
    fd = -float(np.dot(pn, (gp - gm).ravel() / (2 * h)))
    print("k_handle key %.15g differences %.15g restatement %.15g" % (got, fd, sn.k_deriv(x, pn, fv, b, w, t, fz)))
    assert abs(got - fd) <= 1e-8 * abs(fd)
    old = ["cloth0.Kl", "cloth0.Ka", "cloth0.Kb"]
    a = ctx.param_grads(S.pos, S.ref, old, p=p)
    c = ctx.param_grads(S.pos, S.ref, ["k_handle"] + old[:2] + ["k_handle"] + old[2:], p=p)
    assert all(a[k] == c[k] for k in old) and c["k_handle"] == got
    s._close_ctx()


def test_corner_points_equal_the_vertex_handles():
    """a face list of (1, 0, 0)-type points on distinct vertices against the same vertices through tsl_set_handles"""
    rng = np.random.default_rng(33)
    sa, sb = _cloth(12), _cloth(12)
    tab = sa.faces.to_numpy()
    v = rng.permutation(169)[:40].astype(np.int32)
    f = np.array([int(np.nonzero((tab == vi).any(1))[0][0]) for vi in v], np.int32)
    b = (tab[f] == v[:, None]).astype(np.float64)
    assert (b.sum(1) == 1).all()
    w = rng.uniform(0.25, 2.0, len(v))
    dx = sa.cloths[0].dx
    x = sa.pos.to_numpy() + rng.normal(scale=0.15 * dx, size=(169, 3))
    t = x[v] + rng.normal(scale=0.5 * dx, size=(len(v), 3))
    sa.set_surface_handles(f, b, K, w); sb.set_handles(v, K, w)
    pn = rng.normal(size=3 * 169)
    out = []
    for s in (sa, sb):
        s.set_handle_targets(t)
        S = _State(s, x)
        p = _dev(pn)
        out.append(dict(energy=np.array(S.energy()), gradient=S.grad(1), matrix=S.matrix(1), force=S.ctx.handle_force(S.pos), handle_grad=S.ctx.handle_grad(p),
                        k_handle=np.array(S.ctx.param_grads(S.pos, S.ref, ["k_handle"], p=p)["k_handle"]), points=S.ctx.handle_points(S.pos)))
        s._close_ctx()
    for k in out[0]:
        a, c = out[0][k], out[1][k]
        print("%-11s face list against vertex list: max difference %.2e of the largest entry, same bits: %s" % (k, np.abs(a - c).max() / np.abs(c).max(), np.array_equal(a, c)))
        assert np.abs(a - c).max() <= 1e-14 * np.abs(c).max()
    assert np.array_equal(out[0]["points"], x[v])


# ------------------------------------------------------------------------------------------------ off means off
def _assemble_and_step(ctx, x, ref):
    pos = _dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, ref, spd=1, grad=F)
    H = ctx.matrix()[2].copy()
    e = ctx.energy(pos, prev, vel, ref)
    ctx.set_param("contact", 0.0)
    st = ctx.step(pos, prev, vel, ref)
    return F.cpu().numpy(), H, e, pos.cpu().numpy(), vel.cpu().numpy(), st["newton_iters"]


def _grip(c, shift=0.0):
    """(faces, coordinates) of two patches of three face-interior points near the two corners of grid row N"""
    loc = [c.locate(u, v) for u, v in ((0.971, 0.043 + shift), (0.933, 0.071 + shift), (0.953, 0.113 + shift), (0.971, 0.957 - shift), (0.933, 0.929 - shift), (0.953, 0.887 - shift))]
    b = np.array([q for _, q in loc])
    assert (b > 1e-3).all()
    return np.array([f for f, _ in loc], np.int32), b


@pytest.mark.parametrize("how", ["removed", "k_zero"])
def test_off_means_off(how):
    N = 12
    rng = np.random.default_rng(5)
    fresh = _cloth(N, pin=True, perturb=1e-4)
    x = fresh.pos.to_numpy()
    y = x + rng.normal(scale=1e-4, size=x.shape) * (fresh.frozen.to_numpy().reshape(-1, 3) == 0)
    ctx_f = fresh._ensure_ctx()
    ctx_f.set_param("direct", 1)
    want = _assemble_and_step(ctx_f, y, fresh._ref_angle)
    used = _cloth(N, pin=True, perturb=1e-4)
    f, b = _grip(used.cloths[0], 0.3)
    used.set_surface_handles(f, b, K)
    used.set_handle_targets(used.handle_points() + 1e-3)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and np.abs(used.handle_force()).max() > 0
    if how == "removed":
        used.set_surface_handles([], np.zeros((0, 3)), 0.0)
        assert used._ensure_ctx() is ctx_u
    else:
        ctx_u.set_param("k_handle", 0.0)
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, c in zip(want, got):
        assert np.array_equal(a, c)
    fresh._close_ctx(); used._close_ctx()


def test_face_handles_build_no_plan_on_a_direct_path_cloth():
    """N = 32, the smallest grid the auto rule admits to the factorised path (an easy bare cloth stays on the iterative hierarchy under the auto rule, so
    the path is asked for with direct = 1): the plan count with face handles added and moved equals the count without them"""
    counts = []
    for handles in (False, True):
        s = _cloth(32, pin=True, perturb=1e-4)
        ctx = s._ensure_ctx()
        ctx.set_param("direct", 1)
        for step in range(1, 4):
            if handles and step >= 2:
                f, b = _grip(s.cloths[0], 0.2 if step == 2 else 0.25)     # added at step 2, moved to other faces at step 3
                s.set_surface_handles(f, b, 2000.0)
                s.set_handle_targets(s.handle_points() + [0.0, 0.0, 1e-3 * step])
            st = s.time_step(None, step)
            assert st["unconverged"] == 0 and st["factorizations"] > 0
        counts.append(ctx.direct_info()["plans"])
        s._close_ctx()
    assert counts[0] >= 1 and counts[1] == counts[0], counts


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_the_setters_replace_each_other():
    from thinshelllab_amd._lib import TslError
    s = _cloth(12)
    ctx = s._ensure_ctx()
    S = _State(s, s.pos.to_numpy())
    ok_f, ok_b = [3, 3, 17], [[0.2, 0.3, 0.5], [1.0, 0.0, 0.0], [0.0, 0.5, 0.5]]
    ctx.set_handles_on_faces(ok_f, ok_b, [1.0, 2.0, 0.5])
    ctx.set_param("k_handle", K)
    before = ctx.handle_points(S.pos)
    assert before.shape == (3, 3)
    for faces, bary, wts, msg in (
            ([3, 288], ok_b[:2], None, r"face 288 of handle 1 out of range \[0, 288\)"),
            ([-2], ok_b[:1], None, r"face -2 of handle 0 out of range \[0, 288\)"),
            ([3, 4], [ok_b[0], [-0.1, 0.6, 0.5]], None, r"barycentric coordinate -0.1 of handle 1 \(face 4\) is not finite or outside \[0, 1\]"),
            ([3, 4], [ok_b[0], [np.nan, 0.5, 0.5]], None, r"barycentric coordinate nan of handle 1 \(face 4\) is not finite or outside \[0, 1\]"),
            ([3, 4], [ok_b[0], [1.2, 0.0, 0.0]], None, r"barycentric coordinate 1.2 of handle 1 \(face 4\) is not finite or outside \[0, 1\]"),
            ([3], [[0.3, 0.3, 0.3]], None, r"barycentric coordinates \(0.3, 0.3, 0.3\) of handle 0 \(face 3\) sum to 0.9, not 1"),
            ([3, 4], ok_b[:2], [1.0, -1.0], r"weight -1 of handle 1 \(face 4\) is negative or not finite"),
            ([3, 4], ok_b[:2], [np.inf, 1.0], r"weight inf of handle 0 \(face 3\) is negative or not finite")):
        with pytest.raises(TslError, match=msg):
            ctx.set_handles_on_faces(faces, bary, wts)
        assert np.array_equal(ctx.handle_points(S.pos), before)
    # frames on the face list, then a vertex list: the face list and the frames are gone
    ctx.set_handle_frames([0, 0, -1], np.zeros((3, 3)), 1)
    assert ctx.frame_wrench(S.pos).shape == (1, 6)
    ctx.set_handles([5, 9])
    assert ctx.n_frame == 0 and ctx.frame_wrench(S.pos).shape == (0, 6)
    assert np.array_equal(ctx.handle_points(S.pos), s.pos.to_numpy()[[5, 9]]) and ctx.handle_targets().shape == (2, 3) and (ctx.handle_targets() == 0).all()
    ctx.set_handle_frames([0, 0], np.zeros((2, 3)), 1)
    ctx.set_handles_on_faces(ok_f, ok_b)
    assert ctx.n_frame == 0 and ctx.frame_wrench(S.pos).shape == (0, 6) and np.array_equal(ctx.handle_points(S.pos), before) and (ctx.handle_targets() == 0).all()
    ctx.set_handles_on_faces([], np.zeros((0, 3)))
    assert ctx.handle_points(S.pos).shape == (0, 3)
    p = _dev(np.random.default_rng(0).normal(size=3 * s.tot_NV))
    assert ctx.param_grads(S.pos, S.ref, ["k_handle"], p=p)["k_handle"] == 0.0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ frames
def test_frames_on_face_handles():
    """N = 12, 40 face handles on 2 frames plus 3 free ones and an empty third frame"""
    rng = np.random.default_rng(34)
    s = _cloth(12)
    ctx = s._ensure_ctx()
    tab = s.faces.to_numpy()
    n, nf = 43, 3
    f = rng.integers(0, 288, n).astype(np.int32)
    b = rng.dirichlet(np.ones(3), n)
    w = rng.uniform(0.25, 2.0, n)
    frame_of = rng.permutation(np.concatenate([np.zeros(25), np.ones(15), -np.ones(3)])).astype(np.int32)
    local = rng.normal(scale=0.05, size=(n, 3))
    cpos = rng.normal(scale=0.5, size=(nf, 3))
    quat = rng.normal(size=(nf, 4))
    t_world = rng.normal(scale=0.5, size=(n, 3))
    x = s.pos.to_numpy() + rng.normal(scale=0.15 * s.cloths[0].dx, size=(169, 3))
    fz = _frozen_pattern(169, tab[f])
    ctx.set_handles_on_faces(f, b, w)
    ctx.set_param("k_handle", K)
    ctx.set_frozen(fz.reshape(-1))
    ctx.set_handle_targets(t_world)
    ctx.set_handle_frames(frame_of, local, nf)
    ctx.set_frame_poses(cpos, quat)
    t = ctx.handle_targets()
    want = fn.targets(t_world, frame_of, local, cpos, quat)
    print("targets: max |t - (c + R r)| = %.3e m" % np.abs(t - want).max())
    assert np.abs(t - want).max() <= 1e-14 and np.array_equal(t[frame_of < 0], t_world[frame_of < 0])
    pos = _dev(x)
    pn = rng.normal(size=3 * 169)
    p = _dev(pn)
    f_rows, g_rows = ctx.handle_force(pos), ctx.handle_grad(p)
    assert np.abs(f_rows - sn.force(x, tab[f], b, w, t, K)).max() <= 1e-14 * np.abs(f_rows).max()
    assert np.abs(g_rows - sn.target_grad(pn, tab[f], b, w, K, fz)).max() <= 1e-14 * np.abs(g_rows).max()
    for name, got, (ref, mag) in (("wrench", ctx.frame_wrench(pos), fn.wrench(f_rows, t, frame_of, cpos)),
                                  ("grad", ctx.frame_grad(p), fn.pose_grad(g_rows, frame_of, local, quat, nf))):
        rel = np.abs(got - ref) / np.where(mag > 0, mag, 1.0)
        print("frame_%s: max |got - restatement| / sum |terms| = %.3e (bound 1e-12); largest entry %.3e" % (name, rel.max(), np.abs(got).max()))
        assert (np.abs(got - ref) <= 1e-12 * mag).all()
        assert got.shape == (nf, 6) and (got[2] == 0).all() and (got[:2] != 0).all()
    assert np.array_equal(ctx.frame_wrench(pos), ctx.frame_wrench(pos)) and np.array_equal(ctx.frame_grad(p), ctx.frame_grad(p))
    s._close_ctx()
    # grasp where they are, through the scene: every residual is zero
    s = _cloth(12, perturb=1e-3)
    s.set_surface_handles(f, b, K, w)
    s.set_handle_frames(np.maximum(frame_of, 0), n_frames=2)
    s.set_frame_poses(rng.normal(scale=0.3, size=(2, 3)), rng.normal(size=(2, 4)))
    s.set_handle_frames(np.maximum(frame_of, 0))
    ctx = s._ensure_ctx()
    res = ctx.handle_points(s.pos.t) - ctx.handle_targets()
    print("grasp where they are: max residual %.3e m" % np.abs(res).max())
    assert np.abs(res).max() <= 1e-15
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ contact
def test_face_handles_next_to_contact_constraints():
    """Scene_balancing (the three-stream assembly): handles on two cloth faces in contact with the ball and on one surface face of the ball; the
    per-state checks with constraints present, then one forward and one reverse step"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.geometry import projection_query
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=0.06)
    s.init_all()
    s.mu_cloth_elastic[None] = 5.0
    s.prev_pos.copy_from(s.pos)
    n_part = s.gripper.n_part
    dpos = np.zeros((n_part, 3)); drot = np.zeros((n_part, 3))
    dpos[:, 2] = 5e-5; dpos[:, 0] = 2e-4; drot[:, 1] = 2e-3
    for fr in range(1, 3):
        s.action(fr, dpos, drot)
        s.time_step(projection_query, fr)
    ctx = s._ensure_ctx()
    pos, prev, vel, ref = s._state()
    ctx.contact_detect(prev, prev)
    cons = ctx.constraints()
    c, ball = s.cloths[0], s.elastics[0]
    idx = cons["idx"]
    in_contact = np.unique(idx[(idx >= c.offset) & (idx < c.offset + c.NV)])
    assert len(idx) > 0 and len(in_contact) > 0
    tab = s.faces.to_numpy()
    cloth_faces = [int(np.nonzero((tab[:c.NF] == u).any(1))[0][0]) for u in (in_contact[0], in_contact[-1])]
    assert cloth_faces[0] != cloth_faces[1]
    f = np.array(cloth_faces + [ball.offset_faces + 3], np.int32)
    b = np.array([[0.2, 0.5, 0.3], [0.6, 0.0, 0.4], [0.3, 0.3, 0.4]])
    w = np.array([1.0, 0.5, 2.0])
    fv = tab[f]
    assert (fv[2] >= ball.offset).all() and (fv[2] < ball.offset + ball.n_verts).all()
    x = pos.cpu().numpy()
    t = sn.points(x, fv, b) + np.array([[2e-3, -1e-3, 2e-3], [-1e-3, 1e-3, 2e-3], [1e-3, 2e-3, -2e-3]])
    s.set_surface_handles(f, b, K, w)
    s.set_handle_targets(t)
    assert s._ensure_ctx() is ctx
    S = _State(s, x)
    S.prev = prev.clone(); S.vel = vel.clone(); S.ref = ref
    fz = s.frozen.to_numpy().reshape(-1, 3)
    assert not fz[fv].any()
    # (the eigen-clamp of the bodies' element blocks starts from the eigenvectors of the previous assembly, "tet_warm": two assemblies of one
    # state differ in the last bits of the bodies' blocks.  Off for the differences, which ask for exact zeros away from the handles.)
    ctx.set_param("tet_warm", 0)
    _check_state(S, x, fv, b, w, t, fz, False)
    ctx.set_param("tet_warm", 1)
    s.set_surface_handles(f, b, 500.0, w)
    s.set_handle_targets(sn.points(x, fv, b) + 0.1 * (t - sn.points(x, fv, b)))
    g = Grad(s, 2, n_part); g.init_mass(s)
    g.copy_pos(s, 0)
    s.action(3, dpos, drot)
    st = s.time_step(projection_query, 3)
    assert st["unconverged"] == 0 and st["nc"] > 0
    g.copy_pos(s, 1)
    g.pos_grad.t[1] = _dev(np.random.default_rng(13).normal(scale=1e-2, size=(s.tot_NV, 3)))
    g.transfer_grad(1, s, projection_query)
    assert g.last_stats["flag"] != 3 and np.abs(g.handle_grad.t[1].numpy()).min() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ rollouts
# The sheet of DESIGN.md 2.4: 16 x 16, StVK, Kb = 0, flat from rest -- its matrix is the exact second derivative of its energy, so whole-rollout
# gradients can be held to differences.  Two grip patches of three face-interior points near the two corners of grid row N, k = 2000 N/m.
KD = 2000.0
T_TAPE = 6


def _drape(direct=1, handles=True, cg_tol=None):
    s = _cloth(16, pin=not handles, perturb=0.0, Kb=0.0, stvk=(3.0e5, 2.0e5))
    if handles:
        f, b = _grip(s.cloths[0])
        s.set_surface_handles(f, b, KD)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", direct)
    if cg_tol:
        ctx.set_param("cg_tol", cg_tol)
    return s


def _moving_targets(s, T, scale=1.0):
    """per step: up and apart (a membrane without bending stiffness buckles under compression), the two patches differently"""
    p0 = s.handle_points()
    u = p0[3] - p0[0]
    u /= np.linalg.norm(u)
    out = np.cross(u, [0.0, 0.0, 1.0])
    up = np.array([0.0, 0.0, 1.0])
    move = scale * np.array([-1e-4 * u + 3e-4 * up + 1e-4 * out] * 3 + [2e-4 * u + 2e-4 * up] * 3)
    return p0[None] + np.arange(T)[:, None, None] * move[None]


def _reset(s, x0):
    s.pos.from_numpy(x0); s.prev_pos.from_numpy(x0); s.vel.fill(0.0)


def _forward(s, g, targets, T):
    stats = []
    if targets is not None:
        s.set_handle_targets(targets[0])
    g.copy_pos(s, 0)
    for f in range(1, T):
        if targets is not None:
            s.set_handle_targets(targets[f])
        stats.append(s.time_step(None, f))
        g.copy_pos(s, f)
    return stats


def _tape(s, targets, T=T_TAPE):
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    g = Grad(s, T, 0); g.init_mass(s)
    st = _forward(s, g, targets, T)
    assert all(r["unconverged"] == 0 and r["newton_iters"] < 200 for r in st), st
    return g, st


def _reverse(s, g, wgt, T):
    g.pos_grad.t[T - 1] = _dev(wgt)
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3


def test_drape_on_face_handles_repeats_and_group_members_equal_their_single_runs():
    T = T_TAPE
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(289, 3))
    runs = []
    for scale in (1.0, 1.0, 0.5):
        s = _drape()
        g, st = _tape(s, _moving_targets(s, T, scale))
        assert all(r["factorizations"] > 0 for r in st)
        _reverse(s, g, wgt, T)
        assert tuple(g.handle_grad.t.shape) == (T, 6, 3) and tuple(g.handle_targets.t.shape) == (T, 6, 3)
        runs.append((g.pos_buffer.t.cpu().numpy().copy(), g.handle_grad.t.numpy().copy()))
        s._close_ctx()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.abs(runs[0][0][-1] - runs[0][0][0]).max() > 1e-4 and np.abs(runs[0][1][1:]).min() > 0 and not np.array_equal(runs[0][0], runs[2][0])
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.scene_group import SceneGroup
    ms = [_drape(), _drape()]
    tg = [_moving_targets(ms[0], T, 1.0), _moving_targets(ms[1], T, 0.5)]
    G = SceneGroup(ms)
    gs = []
    for m, t in zip(ms, tg):
        g = Grad(m, T, 0); g.init_mass(m)
        m.set_handle_targets(t[0]); g.copy_pos(m, 0)
        gs.append(g)
    for f in range(1, T):
        for m, t in zip(ms, tg):
            m.set_handle_targets(t[f])
        sts = G.time_step(None, f)
        assert all(r["unconverged"] == 0 for r in sts)
        for m, g in zip(ms, gs):
            g.copy_pos(m, f)
    for g in gs:
        g.pos_grad.t[T - 1] = _dev(wgt)
    for f in range(T - 1, 0, -1):
        G.transfer_grad(f, gs, None)
    assert G.info()["merged_factorizations"] > 0
    G.close()
    for i, j in ((0, 0), (1, 2)):
        assert np.array_equal(gs[i].pos_buffer.t.cpu().numpy(), runs[j][0]), i
        assert np.array_equal(gs[i].handle_grad.t.numpy(), runs[j][1]), i
        assert np.array_equal(gs[i].handle_targets.t.numpy(), tg[i]), i
    for m in ms:
        m._close_ctx()


def test_iterative_hierarchy_agrees_with_the_factorised_path():
    """the tape of the drape on face handles with direct = 0 against direct = 1; the bound is the one tests/test_gpu_handles.py uses for its handle
    drape: ten times the same comparison on the drape pinned by its frozen row (no handles)"""
    out = {}
    for handles in (False, True):
        xs = []
        for direct in (1, 0):
            s = _drape(direct=direct, handles=handles)
            g, st = _tape(s, _moving_targets(s, T_TAPE) if handles else None)
            xs.append(g.pos_buffer.t.cpu().numpy().copy())
            s._close_ctx()
        out[handles] = np.abs(xs[0] - xs[1]).max()
    print("max |x_direct - x_iterative| over the tape: pinned row %.3e m, face handles %.3e m" % (out[False], out[True]))
    assert out[True] <= 10 * out[False]


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last state.  sum_s handle_grad[s] . d_s
    against central differences of the loss along d at two step sizes a decade apart, for two random directions d over all targets and steps
    (eight extra rollouts), and grad_params["k_handle"] the same way.  Bound: three times the disagreement of the two differences, which must itself be
    below 1e-2 of the value -- a noisy difference passes nothing.  Step sizes: 1e-6 / 1e-7 m along a direction with entries of order one and 2e-3 / 2e-4
    of k_handle.  At 1e-4 / 1e-5 m the differences disagree by 3 % and by more than their value (the three springs of a patch, moved against each
    other, compress a membrane without bending stiffness, which responds to second order); below 1e-7 m the Newton stop shows.  DESIGN.md 2.6."""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    s = _drape(cg_tol=1e-13)
    x0 = s.pos.to_numpy()
    tg0 = _moving_targets(s, T)
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)

    def rollout(targets, k=KD, reverse=False):
        _reset(s, x0)
        s._ensure_ctx().set_param("k_handle", k)
        g = Grad(s, T, 0); g.init_mass(s)
        g.param_keys = ["k_handle"]
        st = _forward(s, g, targets, T)
        assert all(r["unconverged"] == 0 and r["newton_iters"] < 200 for r in st)
        L = float((g.pos_buffer.t[T - 1].cpu().numpy() * wgt).sum())
        if not reverse:
            return L
        g.pos_grad.t[T - 1] = _dev(wgt)
        for f in range(T - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.pos_grad.t[f - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.handle_grad.t.numpy().copy(), g.grad_params["k_handle"]

    _, hg, gk = rollout(tg0, reverse=True)
    assert hg.shape == (T, 6, 3) and (hg[0] == 0).all()
    checks = []
    for n in range(2):
        d = rng.normal(size=tg0.shape)
        d[0] = 0.0       # (the targets of step 0 enter no step)
        fd = [(rollout(tg0 + h * d) - rollout(tg0 - h * d)) / (2 * h) for h in (1e-6, 1e-7)]
        checks.append(("handle_grad . direction %d" % n, float((hg * d).sum()), fd))
    fk = [(rollout(tg0, KD * (1 + r)) - rollout(tg0, KD * (1 - r))) / (2 * r * KD) for r in (2e-3, 2e-4)]
    checks.append(("k_handle", gk, fk))
    for name, got, fd in checks:
        print("%s: analytic %.10e, differences %.10e / %.10e (disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (name, got, fd[0], fd[1], abs(fd[0] - fd[1]) / abs(fd[1]), abs(got - fd[1]) / abs(fd[1]), 3 * abs(fd[0] - fd[1]) / abs(fd[1])))
    for name, got, fd in checks:
        assert abs(fd[0] - fd[1]) < 1e-2 * abs(fd[1]), name
        assert abs(got - fd[1]) <= 3 * abs(fd[0] - fd[1]), name
    s._close_ctx()


def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_surface_handles import optimise
    losses, steps = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
