"""Ties: vertex-to-face-point springs (tsl_set_ties; csrc/k_tie.hpp) through the C ABI.  The reference has no such term: it is checked
against the dense NumPy restatement (tests/tie_numpy.py), differences of the assembled gradient and whole-rollout differences.  The idiom is that of
tests/test_gpu_surface_handles.py: a tie quantity of a state is the difference against the same state with k_tie = 0 -- no tie slot exists and no tie
kernel runs there, and the rest is formed by the same launches in both -- and K = 2e5 N/m, the size of the cloth's own diagonal entries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ee_numpy as en  # noqa: E402
import tie_numpy as tn  # noqa: E402

pytestmark = pytest.mark.gpu

K = 2.0e5
DX = 0.1 / 15


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _seam(N, k=K, tube=False, perturb=0.0, Kb=100.0, stvk=None, newton_cap=200, sew=True):
    from thinshelllab_amd.task_scene.Scene_seam import Scene
    s = Scene(cloth_size=DX * N, N=N, k_tie=k, tube=tube, Kb=Kb, perturb=perturb, stvk=stvk, newton_cap=newton_cap)
    s.init_all()
    if not sew:
        s.set_ties([], [], np.zeros((0, 3)), 0.0)
    return s


class _State:
    """one state of a context: positions, zero velocity, rest angles; energy / gradient / operator of it as NumPy"""

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

    def operator(self, spd):
        """the full operator, dense: the static matrix plus the masked blocks of every constraint slot (what TslContext.operator_csr builds)"""
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd)
        A = self.ctx.matrix_csr().toarray()
        idx, blk = self.ctx.constraints()["idx"], self.ctx.contact_blocks(True)
        for c in range(len(blk)):
            d = np.concatenate([3 * v + np.arange(3) for v in idx[c]])
            A[np.ix_(d, d)] += blk[c]
        return A

    def tie_part(self, fun, k=K, with_base=False):
        """fun() with k_tie = k minus fun() with k_tie = 0 (with_base: and the latter)"""
        self.ctx.set_param("k_tie", k)
        a = fun()
        self.ctx.set_param("k_tie", 0.0)
        b = fun()
        self.ctx.set_param("k_tie", k)
        return (a - b, b) if with_base else a - b


def _lists(name, s):
    """(vertices, faces, coordinates, weights) on the two 8 x 8 cloths.  seam: the scene's own nine one-hot ties.  dense: 300 ties -- more than one
    256-lane workgroup with a partial wave -- random vertices of cloth 1 on random faces of cloth 0 with Dirichlet coordinates, several per vertex and
    per face, thirty inside cloth 0, one weight 0, one point on an edge.  n65 / one: the first 65 / the first one of them."""
    if name == "seam":
        return s._tie_v.copy(), s._tie_f.copy(), s._tie_b.copy(), None
    rng = np.random.default_rng(41)
    c0, c1 = s.cloths
    tab = s.faces.to_numpy()
    n = 300
    f = rng.integers(c0.offset_faces, c0.offset_faces + c0.NF, n)
    v = rng.integers(c1.offset, c1.offset + c1.NV, n)
    for i in range(270, n):          # inside cloth 0: a vertex of cloth 0 that is no corner of the face
        v[i] = rng.choice(np.setdiff1d(np.arange(c0.offset, c0.offset + c0.NV), tab[f[i]]))
    b = rng.dirichlet(np.ones(3), n)
    w = rng.uniform(0.25, 2.0, n)
    w[5] = 0.0
    b[7] = (0.0, 0.4, 0.6)
    m = {"dense": n, "n65": 65, "one": 1}[name]
    return v[:m].astype(np.int32), f[:m].astype(np.int32), b[:m], w[:m]


def _case(name):
    s = _seam(8)
    assert s.tot_NV == 162 and s.tot_NF == 256
    v, f, b, w = _lists(name, s)
    s.set_ties(v, f, b, K, w)
    s._ensure_ctx().set_gravity(np.zeros((s.tot_NV, 3)))
    s._ensure_ctx().set_param("direct", 1)
    rng = np.random.default_rng({"seam": 1, "dense": 2, "n65": 3, "one": 4}[name])
    x = s.pos.to_numpy() + rng.normal(scale=0.15 * DX, size=(s.tot_NV, 3))
    idx, b, w = tn.records(s.faces.to_numpy(), v, f, b, w)
    return s, x, idx, b, w


def _frozen_pattern(NV, idx):
    """all dofs of one touched vertex, one dof of a second, two of a third"""
    fz = np.zeros((NV, 3), np.int32)
    v0, v1, v2 = idx[0, 3], idx[0, 0], idx[0, 1]
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


def _touched(NV, idx):
    m = np.zeros((3 * NV, 3 * NV), bool)
    for row in idx:
        d = np.concatenate([3 * v + np.arange(3) for v in row])
        m[np.ix_(d, d)] = True
    return m


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", ["seam", "dense", "one", "n65"])
def test_energy_gradient_and_operator_match_the_restatement(name):
    s, x, idx, b, w = _case(name)
    S = _State(s, x)
    ctx, NV, n = S.ctx, s.tot_NV, len(idx)
    assert ctx.tie_count() == n and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == n
    cons = ctx.constraints()
    assert np.array_equal(cons["idx"], idx) and np.array_equal(cons["w"], b) and not cons["k"].any() and not cons["mu"].any() and not cons["T"].any()
    e_np, g_np, H_np = tn.energy(x, idx, b, w, K), tn.gradient(x, idx, b, w, K), tn.hessian(NV, idx, b, w, K)
    B_np = tn.blocks(b, w, K)
    inside = _touched(NV, idx)
    for frozen in (np.zeros((NV, 3), np.int32), _frozen_pattern(NV, idx)):
        ctx.set_frozen(frozen.reshape(-1))
        fzb = frozen.astype(bool)
        free = (~fzb).ravel()
        e = S.tie_part(S.energy)
        print("%s: energy %.17g restatement %.17g rel %.2e" % (name, e, e_np, abs(e - e_np) / abs(e_np)))
        assert abs(e - e_np) <= 1e-12 * abs(e_np)
        g = S.tie_part(S.grad)
        gm = g_np * ~fzb
        print("gradient err / max %.2e" % (np.abs(g - gm).max() / np.abs(gm).max()))
        assert np.abs(g - gm).max() <= 1e-12 * np.abs(gm).max() and (g[fzb] == 0).all()
        Hm = H_np * np.outer(free, free)
        full = []
        for spd in (0, 1, 2):
            D, A = S.tie_part(lambda spd=spd: S.operator(spd), with_base=True)
            print("spd %d: operator err / largest tie entry %.2e, asymmetric entries of the difference / of the rest %d / %d"
                  % (spd, np.abs(D - Hm).max() / np.abs(Hm).max(), (D != D.T).sum(), (A != A.T).sum()))
            assert np.abs(D - Hm).max() <= 1e-12 * np.abs(Hm).max()
            assert (D[~inside] == 0).all() and (D[~free] == 0).all() and (D[:, ~free] == 0).all()
            assert not ((D != D.T) & (A == A.T)).any()
            blk_full, blk_m = ctx.contact_blocks(False), ctx.contact_blocks(True)
            assert blk_full.shape == (n, 12, 12) and np.array_equal(blk_full, blk_full.transpose(0, 2, 1)) and np.array_equal(blk_m, blk_m.transpose(0, 2, 1))
            assert np.abs(blk_full - B_np).max() <= 1e-12 * np.abs(B_np).max()
            full.append(blk_full)
        assert np.array_equal(full[0], full[1]) and np.array_equal(full[0], full[2])          # the three spd modes: the same tie blocks
    if name == "seam":          # the interface's own operator
        ctx.assemble(S.pos, S.prev, S.vel, S.ref, spd=1)
        assert np.array_equal(ctx.operator_csr().toarray(), S.operator(1))
    s._close_ctx()


@pytest.mark.parametrize("name", ["seam", "dense"])
def test_read_outs_and_stiffness_key(name):
    s, x, idx, b, w = _case(name)
    S = _State(s, x)
    ctx, NV = S.ctx, s.tot_NV
    fz = _frozen_pattern(NV, idx)
    ctx.set_frozen(fz.reshape(-1))
    r, r_np = ctx.tie_residuals(S.pos), tn.residuals(x, idx, b)
    fo, fo_np = ctx.tie_force(S.pos), tn.force(x, idx, b, w, K)
    assert np.abs(r - r_np).max() <= 1e-14 * np.abs(r_np).max() and np.abs(fo - fo_np).max() <= 1e-14 * np.abs(fo_np).max()
    pn = np.random.default_rng(11).normal(size=3 * NV)
    p = _dev(pn)
    rows = tn.pg_rows(x, pn, fz, idx, b)
    tg = ctx.tie_grad(S.pos, p)
    print("residuals %.2e, force %.2e, tie_grad %.2e of the largest entry" % (np.abs(r - r_np).max() / np.abs(r_np).max(),
          np.abs(fo - fo_np).max() / np.abs(fo_np).max(), np.abs(tg - K * rows).max() / np.abs(K * rows).max()))
    assert np.abs(tg - K * rows).max() <= 1e-14 * np.abs(K * rows).max()
    # the k_tie key against central differences of the assembled (masked) gradient: the term is linear in k_tie
    got = ctx.param_grads(S.pos, S.ref, ["k_tie"], p=p)["k_tie"]
    h = 0.5 * K
    ctx.set_param("k_tie", K + h); gp = S.grad()
    ctx.set_param("k_tie", K - h); gm = S.grad()
    ctx.set_param("k_tie", K)
    fd = -float(np.dot(pn, (gp - gm).ravel() / (2 * h)))
    print("k_tie key %.15g differences %.15g restatement %.15g" % (got, fd, float(w @ rows)))
    assert abs(got - fd) <= 1e-8 * abs(fd)
    ident = float(w @ tg)
    assert abs(K * got - ident) <= 1e-13 * abs(ident), (K * got, ident)
    old = ["cloth0.Kl", "cloth0.Ka", "cloth1.Kb", "k_handle"]
    a = ctx.param_grads(S.pos, S.ref, old, p=p)
    c = ctx.param_grads(S.pos, S.ref, ["k_tie"] + old[:2] + ["k_tie"] + old[2:], p=p)
    assert all(a[k] == c[k] for k in old) and c["k_tie"] == got and a["cloth0.Kl"] != 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ three slot classes at once
def _bars():
    """the smallest scene of tests/test_gpu_contact_ee.py with vertex-triangle and edge-edge slots live: the coarse tangled bars"""
    rng = np.random.default_rng(11)
    sc = en.bar_scene(n=6, dx=0.01, w=0.01, gap=-3e-3, angle=np.pi / 3)
    x = sc["x"] + rng.normal(scale=1.5e-3, size=sc["x"].shape)
    return sc, x


def _bar_ties(sc):
    """vertices of the upper bar onto surface faces of the lower one"""
    nl, tab = sc["n_lower"], np.asarray(sc["faces"]).reshape(-1, 3)
    lower_faces = [f for f in range(len(tab)) if (tab[f] < nl).all()]
    rng = np.random.default_rng(3)
    f = rng.choice(lower_faces, 7)
    v = rng.integers(nl, len(sc["x"]), 7)
    return v.astype(np.int32), f.astype(np.int32), rng.dirichlet(np.ones(3), 7), rng.uniform(0.5, 1.5, 7)


def test_ties_behind_vertex_triangle_and_edge_edge_slots():
    sc, x = _bars()
    NV = len(x)
    pos = _dev(x)
    zero3 = torch.zeros(3, dtype=torch.float64, device="cuda")
    out = {}
    for ties in (False, True):
        ctx = en.bar_context(sc, eps_contact=2e-3)
        ctx.set_param("contact_ee", 1)
        ctx.set_param("direct", 1)
        if ties:
            v, f, b, w = _bar_ties(sc)
            ctx.set_ties(v, f, b, w)
            ctx.set_param("k_tie", 500.0)
        ctx.contact_detect(pos, pos.clone())
        counts = ctx.contact_counts()
        ctx.assemble(pos, pos.clone(), torch.zeros_like(pos), zero3, spd=1)
        p = _dev(np.random.default_rng(5).normal(size=3 * NV))
        with pytest.raises(Exception, match="k_contact: .* edge-edge constraints"):
            ctx.param_grads(pos, zero3, ["k_contact"], p=p)
        rec = dict(counts=counts, n=ctx.tie_count(), cons=ctx.constraints(), blk=ctx.contact_blocks(False), blk_m=ctx.contact_blocks(True))
        # vertex-triangle slots alone: the k_contact key is allowed, with and without ties
        ctx.set_param("contact_ee", 0)
        ctx.contact_detect(pos, pos.clone())
        assert ctx.contact_counts()[1] == 0
        rec["counts_vf"] = ctx.contact_counts()
        rec["k_contact"] = ctx.param_grads(pos, zero3, ["k_contact"] + (["k_tie"] if ties else []), p=p)["k_contact"]
        ctx.set_param("contact_ee", 1)
        # one forward and one reverse step
        xs = [pos.clone()]
        q, prev, vel = pos.clone(), pos.clone(), torch.zeros_like(pos)
        st = ctx.step(q, prev, vel, zero3)
        assert st["unconverged"] == 0, st
        xs.append(q.clone())
        pb = torch.stack(xs).contiguous(); pg = torch.zeros_like(pb)
        pg[1] = _dev(np.random.default_rng(6).normal(scale=1e-2, size=(NV, 3)))
        rb = torch.zeros((2, 3), dtype=torch.float64, device="cuda"); ag = torch.zeros_like(rb)
        tz = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
        ast = ctx.adjoint_step(1, 2, pb, pg, rb, ag, tz, 1.0)
        assert ast["flag"] != 3, ast
        out[ties] = rec
        ctx.close()
    a, t = out[False], out[True]
    n_vf, n_ee = a["counts"]
    print("slots: %d vertex-triangle, %d edge-edge, %d ties" % (n_vf, n_ee, t["n"]))
    assert n_vf > 0 and n_ee > 0 and t["counts"] == a["counts"] and t["counts_vf"] == a["counts_vf"] and a["counts_vf"][0] > 0 and (a["n"], t["n"]) == (0, 7)
    m = n_vf + n_ee
    assert len(a["cons"]["idx"]) == m and len(t["cons"]["idx"]) == m + 7
    for k in a["cons"]:
        assert np.array_equal(a["cons"][k], t["cons"][k][:m]), k
    assert np.array_equal(a["blk"], t["blk"][:m]) and np.array_equal(a["blk_m"], t["blk_m"][:m])
    v, f, b, w = _bar_ties(sc)
    idx, b, w = tn.records(np.asarray(sc["faces"]).reshape(-1, 3), v, f, b, w)
    assert np.array_equal(t["cons"]["idx"][m:], idx)
    B = tn.blocks(b, w, 500.0)
    assert np.abs(t["blk"][m:] - B).max() <= 1e-12 * np.abs(B).max()
    assert a["k_contact"] == t["k_contact"] and a["k_contact"] != 0


# ------------------------------------------------------------------------------------------------ off means off
def _drape(N=12):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=DX * N, N=N, M=N, pin_row=True, perturb=1e-4, newton_cap=200)
    s.init_all()
    return s


def _assemble_and_step(ctx, x, ref):
    pos = _dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, ref, spd=1, grad=F)
    H = ctx.operator_csr().toarray()
    e = ctx.energy(pos, prev, vel, ref)
    ctx.set_param("contact", 0.0)
    st = ctx.step(pos, prev, vel, ref)
    return F.cpu().numpy(), H, e, pos.cpu().numpy(), vel.cpu().numpy(), st["newton_iters"]


def _local_ties(s, n=300):
    """n ties inside the drape cloth: vertex (i, j) onto a face two rows further on, so that the cloth is folded nowhere"""
    c = s.cloths[0]
    tab = s.faces.to_numpy()
    rng = np.random.default_rng(9)
    W = c.M + 1
    v = rng.integers(0, (c.N - 3) * W, n)
    f = np.array([rng.choice(np.nonzero((tab == vi + 2 * W).any(axis=1))[0]) for vi in v])
    return v.astype(np.int32), f.astype(np.int32), rng.dirichlet(np.ones(3), n), rng.uniform(0.5, 1.5, n)


@pytest.mark.parametrize("how", ["removed", "k_zero"])
def test_off_means_off_and_300_ties_fit_a_scene_with_cap_16(how):
    rng = np.random.default_rng(5)
    fresh = _drape()
    assert fresh.max_n_constraints == 16
    x = fresh.pos.to_numpy()
    y = x + rng.normal(scale=1e-4, size=x.shape) * (fresh.frozen.to_numpy().reshape(-1, 3) == 0)
    ctx_f = fresh._ensure_ctx()
    ctx_f.set_param("direct", 1)
    want = _assemble_and_step(ctx_f, y, fresh._ref_angle)
    used = _drape()
    v, f, b, w = _local_ties(used)
    used.set_ties(v, f, b, 200.0, w)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and ctx_u.tie_count() == 300 and len(ctx_u.constraints()["idx"]) == 300 and ctx_u.contact_counts() == (0, 0)
    assert np.abs(used.tie_force()).max() > 0 and ctx_u.contact_blocks().shape == (300, 12, 12)
    if how == "removed":
        used.set_ties([], [], np.zeros((0, 3)), 0.0)
        assert used._ensure_ctx() is ctx_u and ctx_u.tie_count() == 0
    else:
        ctx_u.set_param("k_tie", 0.0)
    assert len(ctx_u.constraints()["idx"]) == 0
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, c in zip(want, got):
        assert np.array_equal(a, c)
    fresh._close_ctx(); used._close_ctx()


def test_a_detection_over_the_cap_still_fails_with_its_message():
    sc, x = _bars()
    ctx = en.bar_context(sc, eps_contact=2e-3, max_n_constraints=2)
    ctx.set_param("contact_ee", 1)
    v, f, b, w = _bar_ties(sc)
    ctx.set_ties(v, f, b, w)
    ctx.set_param("k_tie", 500.0)
    pos = _dev(x)
    with pytest.raises(Exception, match=r"contact detection: \d+ vertex-triangle \+ \d+ edge-edge active constraints exceed max_n_constraints = 2 \(raise the scene's max_n_constraints\)"):
        ctx.contact_detect(pos, pos.clone())
    ctx.close()
    ctx = en.bar_context(sc, eps_contact=2e-3, max_n_constraints=1)          # (the state holds two vertex-triangle constraints)
    ctx.set_ties(v, f, b, w)
    ctx.set_param("k_tie", 500.0)
    with pytest.raises(Exception, match=r"contact detection: 2 active constraints exceed max_n_constraints = 1 \(raise the scene's max_n_constraints\)"):
        ctx.contact_detect(pos, pos.clone())
    ctx.close()


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("contact", [0, 1])
def test_seam_plans_are_built_once(contact):
    """N = 32 per cloth, the smallest grid the auto rule admits to the factorised path, asked for with direct = 1: the plan count after the first step
    does not grow over the rollout, and the reverse sweep builds no plan"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    T = 4
    s = _seam(32, perturb=1e-4, newton_cap=50)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    fc = 1 if contact else None
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    plans = []
    for f in range(1, T):
        st = s.time_step(fc, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0, st
        g.copy_pos(s, f)
        plans.append(ctx.direct_info()["plans"])
    assert plans[0] >= 1 and plans[-1] == plans[0], plans
    g.pos_grad.t[T - 1] = _dev(np.random.default_rng(7).normal(scale=1e-2, size=(s.tot_NV, 3)))
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, fc)
        assert g.last_stats["flag"] != 3
    assert ctx.direct_info()["plans"] == plans[0], (ctx.direct_info()["plans"], plans)
    assert ctx.tie_count() == 33 and tuple(g.tie_grad.t.shape) == (T, 33)
    s._close_ctx()


def test_tube_factorises():
    s = _seam(32, tube=True, newton_cap=50)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    for f in range(1, 3):
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0, st
    assert ctx.tie_count() == 33 and ctx.direct_info()["plans"] >= 1
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ rollouts
STVK = (3.0e5, 2.0e5)
T_TAPE = 6


def _hang(k=K, direct=1, sew=True):
    s = _seam(12, k=k, Kb=0.0, stvk=STVK, sew=sew)
    s._ensure_ctx().set_param("direct", direct)
    return s


def _tape(s, T=T_TAPE, wgt=None):
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    rmax = 0.0
    for f in range(1, T):
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["newton_iters"] < 200, st
        g.copy_pos(s, f)
        if s.n_tie:
            rmax = max(rmax, float(np.abs(s.tie_residuals()).max()))
    if wgt is not None:
        g.pos_grad.t[T - 1] = _dev(wgt)
        for f in range(T - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.last_stats["flag"] != 3
    return g, rmax


def test_hanging_cloth_stays_attached_repeats_and_group_members_equal_their_single_runs():
    """max |r_i| over the rollout against ten times the static estimate m g / (k w): m the mass of the hanging cloth per tie, w = 1"""
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(2 * 169, 3))
    runs = {}
    for tag, k in (("a", K), ("b", K), ("half", 0.5 * K)):
        s = _hang(k)
        c1 = s.cloths[1]
        m = float(s.mass.to_numpy()[c1.offset:c1.offset + c1.NV].sum()) / s.n_tie
        g, rmax = _tape(s, wgt=wgt)
        print("k_tie %.3g: max |r_i| = %.3e m, static estimate m g / k = %.3e m" % (k, rmax, m * 9.8 / k))
        assert 0 < rmax < 10 * m * 9.8 / k
        runs[tag] = (g.pos_buffer.t.cpu().numpy().copy(), g.pos_grad.t.cpu().numpy().copy(), g.tie_grad.t.numpy().copy())
        s._close_ctx()
    for a, b in zip(runs["a"], runs["b"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(runs["a"][0], runs["half"][0]) and np.abs(runs["a"][2][1:]).max() > 0 and (runs["a"][2][0] == 0).all()
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.scene_group import SceneGroup
    ms = [_hang(K), _hang(0.5 * K)]
    G = SceneGroup(ms)
    gs = []
    for m_ in ms:
        g = Grad(m_, T_TAPE, 0); g.init_mass(m_); g.copy_pos(m_, 0)
        gs.append(g)
    for f in range(1, T_TAPE):
        sts = G.time_step(None, f)
        assert all(r["unconverged"] == 0 for r in sts)
        for m_, g in zip(ms, gs):
            g.copy_pos(m_, f)
    for g in gs:
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
    for f in range(T_TAPE - 1, 0, -1):
        G.transfer_grad(f, gs, None)
    assert G.info()["merged_factorizations"] > 0
    G.close()
    for i, tag in ((0, "a"), (1, "half")):
        assert np.array_equal(gs[i].pos_buffer.t.cpu().numpy(), runs[tag][0]), i
        assert np.array_equal(gs[i].pos_grad.t.cpu().numpy(), runs[tag][1]), i
        assert np.array_equal(gs[i].tie_grad.t.numpy(), runs[tag][2]), i
    for m_ in ms:
        m_._close_ctx()


def test_iterative_hierarchy_agrees_with_the_factorised_path():
    """the tape of the hanging cloth with direct = 0 against direct = 1, within ten times the same comparison without ties (the rule of DESIGN.md 2.4)"""
    out = {}
    for sew in (False, True):
        xs = []
        for direct in (1, 0):
            s = _hang(direct=direct, sew=sew)
            g, _ = _tape(s)
            xs.append(g.pos_buffer.t.cpu().numpy().copy())
            s._close_ctx()
        out[sew] = np.abs(xs[0] - xs[1]).max()
    print("max |x_direct - x_iterative| over the tape: without ties %.3e m, sewn %.3e m" % (out[False], out[True]))
    assert out[True] <= 10 * out[False]


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last state of the hanging cloth.
    grad_params["k_tie"], sum_s tie_grad[s] . d along two random weight directions d, and pos_grad[0] . e along a random direction e over the free
    dofs of the start state (the state before it held fixed, as the tape defines row 0), each against central differences at two steps a decade apart.  Bound: three times the disagreement of the two
    differences, which must itself be below 1e-2 of the value (the rule of tests/test_gpu_surface_handles.py).  Steps: 2e-3 / 2e-4 of k_tie, 1e-2 /
    1e-3 in the weights (of size 1), 1e-7 / 1e-8 m in the positions (at 1e-6 / 1e-7 m the two differences disagree by 1.4 %: the start velocity h e / dt
    folds the membrane to second order).  DESIGN.md 2.7."""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    KH = 2000.0          # (a seam soft enough that its stretch, m g / k of some 1e-5 m, shows in the loss)
    s = _hang(KH)
    ctx = s._ensure_ctx()
    ctx.set_param("cg_tol", 1e-13)
    x0 = s.pos.to_numpy()
    v, f, b = s._tie_v.copy(), s._tie_f.copy(), s._tie_b.copy()
    w0 = np.ones(len(v))
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)
    free = s.frozen.to_numpy().reshape(-1, 3) == 0

    def rollout(k=KH, w=w0, x=x0, reverse=False):
        s.set_ties(v, f, b, k, w)
        # the tape's row 0 is d(loss)/d(x_0) with the state before it held fixed (k_adj_prev: x_hat_1 = x_0 + damping (x_0 - x_-1)), so the start
        # velocity moves with the start state: vel_0 = damping (x_0 - x_-1) / dt, x_-1 the unperturbed start
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.from_numpy((x - x0) * (s.damping / s.dt))
        g = Grad(s, T, 0); g.init_mass(s)
        g.count_kb_grad = False
        g.param_keys = ["k_tie"]
        g.copy_pos(s, 0)
        for fr in range(1, T):
            st = s.time_step(None, fr)
            assert st["unconverged"] == 0 and st["newton_iters"] < 200
            g.copy_pos(s, fr)
        L = float((g.pos_buffer.t[T - 1].cpu().numpy() * wgt).sum())
        if not reverse:
            return L
        g.pos_grad.t[T - 1] = _dev(wgt)
        for fr in range(T - 1, 0, -1):
            g.transfer_grad(fr, s, None)
            assert g.pos_grad.t[fr - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.tie_grad.t.numpy().copy(), g.grad_params["k_tie"], g.pos_grad.t[0].cpu().numpy().copy()

    _, tg, gk, pg0 = rollout(reverse=True)
    assert tg.shape == (T, len(v)) and (tg[0] == 0).all()
    checks = [("k_tie", gk, [(rollout(k=KH * (1 + r)) - rollout(k=KH * (1 - r))) / (2 * r * KH) for r in (2e-3, 2e-4)])]
    for n in range(2):
        d = rng.uniform(-1.0, 1.0, len(v))
        checks.append(("tie_grad . direction %d" % n, float((tg.sum(0) * d).sum()), [(rollout(w=w0 + h * d) - rollout(w=w0 - h * d)) / (2 * h) for h in (1e-2, 1e-3)]))
    e = rng.normal(size=x0.shape) * free
    checks.append(("pos_grad[0] . direction", float((pg0 * e).sum()), [(rollout(x=x0 + h * e) - rollout(x=x0 - h * e)) / (2 * h) for h in (1e-7, 1e-8)]))
    for name, got, fd in checks:
        print("%s: analytic %.10e, differences %.10e / %.10e (disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (name, got, fd[0], fd[1], abs(fd[0] - fd[1]) / abs(fd[1]), abs(got - fd[1]) / abs(fd[1]), 3 * abs(fd[0] - fd[1]) / abs(fd[1])))
    for name, got, fd in checks:
        assert abs(fd[0] - fd[1]) < 1e-2 * abs(fd[1]), name
        assert abs(got - fd[1]) <= 3 * abs(fd[0] - fd[1]), name
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_keep_the_previous_list():
    s = _seam(8)
    ctx = s._ensure_ctx()
    pos = s.pos.t
    x = s.pos.to_numpy() + np.random.default_rng(3).normal(scale=1e-3, size=(s.tot_NV, 3))
    pos = _dev(x)
    before = ctx.tie_residuals(pos)
    assert before.shape == (9, 3) and np.abs(before).max() > 0
    NV, NF = s.tot_NV, s.tot_NF
    tab = s.faces.to_numpy()
    good_b = [0.2, 0.3, 0.5]
    cases = [((100, NF, good_b, 1.0), rf"face {NF} of tie 1 out of range \[0, {NF}\)"),
             ((100, -1, good_b, 1.0), rf"face -1 of tie 1 out of range \[0, {NF}\)"),
             ((NV, 5, good_b, 1.0), rf"vertex {NV} of tie 1 \(face 5\) out of range \[0, {NV}\)"),
             ((int(tab[5][2]), 5, good_b, 1.0), rf"vertex {int(tab[5][2])} of tie 1 is a corner of its own face 5"),
             ((100, 5, [-0.1, 0.6, 0.5], 1.0), r"barycentric coordinate -0.1 of tie 1 \(face 5, vertex 100\) is not finite or outside \[0, 1\]"),
             ((100, 5, [np.nan, 0.5, 0.5], 1.0), r"barycentric coordinate nan of tie 1 \(face 5, vertex 100\) is not finite or outside \[0, 1\]"),
             ((100, 5, [0.3, 0.3, 0.3], 1.0), r"barycentric coordinates \(0.3, 0.3, 0.3\) of tie 1 \(face 5, vertex 100\) sum to 0.9, not 1"),
             ((100, 5, good_b, -1.0), r"weight -1 of tie 1 \(face 5, vertex 100\) is negative or not finite"),
             ((100, 5, good_b, np.inf), r"weight inf of tie 1 \(face 5, vertex 100\) is negative or not finite")]
    for (v, f, b, w), pat in cases:
        with pytest.raises(Exception, match="tsl_set_ties: " + pat):
            ctx.set_ties([120, v], [7, f], [good_b, b], [1.0, w])
        with pytest.raises(ValueError, match="set_ties: " + pat):          # the scene's host check: the library's message
            s.set_ties([120, v], [7, f], [good_b, b], 10.0, [1.0, w])
        assert ctx.tie_count() == 9 and np.array_equal(ctx.tie_residuals(pos), before)
    with pytest.raises(Exception, match="k_tie must be finite and >= 0"):
        ctx.set_param("k_tie", -1.0)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ driver
def test_sysid_driver_lowers_the_loss():
    from thinshelllab_amd.training.sysid_seam import optimise
    losses, ks = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
