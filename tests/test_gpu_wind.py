"""Wind (tsl_set_wind; csrc/k_wind.hpp) through the C ABI.  The reference has no such term: it is checked against the dense NumPy
restatement (tests/wind_numpy.py), closed forms (total momentum of a free sheet, the isotropic limit, a tangential wind) and whole-rollout
differences.  The idiom is that of tests/test_gpu_spheres.py: a wind quantity of a state is the difference against the same state with
wind_cn = wind_ct = 0 -- no wind kernel runs there, and the rest is formed by the same launches in both.  The restatement checks run with
coefficients of 4e8 and 1e8 N s / m^3, which put the wind blocks M / (9 dt) at the size of the cloth's own diagonal entries (2e5 N / m), so that the
difference of two operators carries the wind part to the last bits; the physical checks use coefficients of the order of 1e2."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wind_numpy as wn  # noqa: E402

pytestmark = pytest.mark.gpu

CN, CT = 4.0e8, 1.0e8
DX = 0.1 / 15
W0 = np.array([0.31, -0.17, 0.23])


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


class _State:
    """one state of a context: positions, start-of-step positions, zero velocity, rest angles; energy / gradient / operator of it as NumPy"""

    def __init__(self, ctx, x, xp, ref, cn=CN, ct=CT):
        self.ctx = ctx
        self.pos = _dev(x); self.prev = _dev(xp); self.vel = torch.zeros_like(self.pos)
        self.ref = ref
        self.cn, self.ct = cn, ct

    def energy(self):
        return self.ctx.energy(self.pos, self.prev, self.vel, self.ref)

    def grad(self, spd=0):
        F = torch.zeros(self.pos.numel(), dtype=torch.float64, device="cuda")
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd, grad=F)
        return F.cpu().numpy().reshape(-1, 3)

    def operator(self, spd):
        self.ctx.assemble(self.pos, self.prev, self.vel, self.ref, spd=spd)
        return self.ctx.operator_csr().toarray()

    def on(self, yes=True):
        self.ctx.set_param("wind_cn", self.cn if yes else 0.0)
        self.ctx.set_param("wind_ct", self.ct if yes else 0.0)

    def part(self, fun, with_base=False):
        """fun() with the wind on minus fun() with wind_cn = wind_ct = 0 (with_base: and the latter)"""
        self.on(True)
        a = fun()
        self.on(False)
        b = fun()
        self.on(True)
        return (a - b, b) if with_base else a - b


def _drape(N, pin=True, perturb=0.0, newton_cap=200):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=DX * N, N=N, M=N, pin_row=pin, perturb=perturb, newton_cap=newton_cap)
    s.init_all()
    return s


def _moved(x0, sel, seed):
    """(x_prev, x): the vertices `sel` moved out of their places by dx / 20, then by about dx / 10 over the step"""
    rng = np.random.default_rng(seed)
    xp, x = x0.copy(), x0.copy()
    xp[sel] += rng.normal(scale=DX / 20, size=(len(sel), 3))
    x[sel] = xp[sel] + rng.normal(scale=DX / 10, size=(len(sel), 3))
    return xp, x


def _wind_list(face_ids, seed):
    """four fifths of the faces `face_ids`, shuffled, with weights in [0.5, 2] of which every seventh is exactly 0"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.asarray(face_ids))[: (4 * len(face_ids)) // 5].astype(np.int32)
    w = rng.uniform(0.5, 2.0, len(ids))
    w[::7] = 0.0
    assert (np.diff(ids) < 0).any() and (w == 0).sum() >= 3
    return ids, w


def _frozen_pattern(fz0, touched):
    """on top of the scene's own frozen dofs: all dofs of one listed corner, one dof of a second, two of a third"""
    fz = fz0.copy()
    v0, v1, v2 = touched[:3]
    fz[v0] = 1
    fz[v1, 1] = 1
    fz[v2, 0] = 1; fz[v2, 2] = 1
    return fz


def _reverse_step(S, NV, n_ref, mass, dt, frozen):
    """One reverse step (step 2 of a tape of three states x_0 = x_1 = x_prev, x_2 = x) with a random right-hand side.  Returns (the adjoint solution p
    on its free dofs, the wind's share of pos_grad[1], wind_grad of that solution).  k_adj_prev adds (1 + d) p m / dt^2 to pos_grad[1] and subtracts
    d p m / dt^2 from pos_grad[0] (d = 1, nothing else writes pos_grad[0], and with contact off only the wind writes pos_grad[1] besides): p is
    read off pos_grad[0] with three roundings, and the wind's share is pos_grad[1] + 2 pos_grad[0]."""
    ctx = S.ctx
    pb = torch.stack([S.prev, S.prev, S.pos]).contiguous()
    pg = torch.zeros_like(pb)
    pg[2] = _dev(np.random.default_rng(6).normal(scale=1e-2, size=(NV, 3)))
    rb = torch.stack([S.ref[:n_ref].reshape(-1)] * 3).contiguous(); ag = torch.zeros_like(rb)
    tz = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
    st = ctx.adjoint_step(2, 3, pb, pg, rb, ag, tz, 1.0)
    assert st["flag"] != 3, st
    out = pg.cpu().numpy().reshape(3, NV, 3)
    free = frozen == 0
    p = np.where(free, -out[0] * (dt * dt) / mass[:, None], 0.0)
    assert not out[0][~free].any() and not out[1][~free].any()
    return p, out[1] + 2.0 * out[0], ctx.wind_grad(S.pos, S.prev)


def _check_state(S, s, x, xp, faces_tab, ids, w, fz_list, n_ref):
    """energy, gradient, operator in the spd modes 0, 1, 2 and with spd_literal, the read-outs and one reverse step of one state against the
    restatement.  Bound: 1e-12 of the largest entry of the restated quantity."""
    ctx = S.ctx
    NV = len(x)
    dt = s.dt
    F = faces_tab[ids]
    args = (F, w, W0, CN, CT, dt)
    assert ctx.wind_count() == len(ids)
    e_np, g_np, H_np = wn.energy(x, xp, *args), wn.gradient(x, xp, *args), wn.hessian(x, xp, *args)
    inside = np.zeros((3 * NV, 3 * NV), bool)
    for f in F:
        for a in f:
            for b in f:
                inside[3 * a:3 * a + 3, 3 * b:3 * b + 3] = True
    mass = s.mass.to_numpy()
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
        Hm = H_np * ff
        big = np.abs(Hm).max()
        got = {}
        for tag, spd, lit in (("spd 0", 0, 0), ("spd 1", 1, 0), ("spd 2", 2, 0), ("literal", 1, 1)):
            ctx.set_param("spd_literal", lit)
            D, A = S.part(lambda spd=spd: S.operator(spd), with_base=True)
            ctx.set_param("spd_literal", 0)
            print("%s: operator err / largest wind entry %.2e, asymmetric entries of the difference / of the rest %d / %d"
                  % (tag, np.abs(D - Hm).max() / big, (D != D.T).sum(), (A != A.T).sum()))
            assert np.abs(D - Hm).max() <= 1e-12 * big
            assert (D[~inside] == 0).all() and (D[~free] == 0).all() and (D[:, ~free] == 0).all()
            assert not ((D != D.T) & (A == A.T)).any()          # the wind part is symmetric bit for bit
            got[tag] = (D, A)
        # every mode adds the same numbers: the same bits wherever the rest of the operator has the same bits in both
        for tag in ("spd 0", "spd 2", "literal"):
            D1, A1 = got["spd 1"]; D2, A2 = got[tag]
            same = (A1 == A2) & inside
            print("%s against spd 1: %d of %d entries of the touched blocks lie on equal bits of the rest; largest difference %.2e of the largest wind entry"
                  % (tag, same.sum(), inside.sum(), np.abs(D1 - D2).max() / big))
            assert (D1[same] == D2[same]).all() and np.abs(D1 - D2).max() <= 1e-12 * big
        # the read-outs (frozen dofs: not masked in the force, not counted in the gradient)
        fo, fo_np = ctx.wind_force(S.pos, S.prev), wn.wind_force(x, xp, *args)
        pn = np.random.default_rng(11).normal(size=(NV, 3))
        wg, wg_np = ctx.wind_grad(S.pos, S.prev, _dev(pn.reshape(-1))), wn.wind_grad(x, xp, pn, frozen, *args)
        print("force %.2e of its largest entry" % (np.abs(fo - fo_np).max() / np.abs(fo_np).max()))
        assert np.abs(fo - fo_np).max() <= 1e-12 * np.abs(fo_np).max() and np.abs(fo_np).min() > 0
        for lo, hi in ((0, 3), (3, 4), (4, 5)):
            print("  wind_grad[%d:%d] %.2e of its largest entry" % (lo, hi, np.abs(wg - wg_np)[lo:hi].max() / np.abs(wg_np[lo:hi]).max()))
            assert np.abs(wg - wg_np)[lo:hi].max() <= 1e-12 * np.abs(wg_np[lo:hi]).max()
        assert np.abs(wg_np).min() > 0
        # one reverse step: the wind's share of pos_grad[s-1], and the read-out of the step's own adjoint solution
        p, share, wg2 = _reverse_step(S, NV, n_ref, mass, dt, frozen)
        want = wn.backprop_prev(x, xp, p, frozen, *args)
        print("pos_grad[s-1] err / max %.2e (largest entry %.3e)" % (np.abs(share - want).max() / np.abs(want).max(), np.abs(want).max()))
        assert np.abs(share - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0
        wg2_np = wn.wind_grad(x, xp, p, frozen, *args)
        assert np.abs(wg2 - wg2_np).max() <= 1e-12 * np.abs(wg2_np).max()


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("N", [8, 20])
def test_bare_cloth_matches_the_restatement(N):
    """N = 8: 81 vertices, 128 faces on the single-stream path, one partial workgroup; N = 20: 441 vertices, 800 faces of which 640 are listed --
    three face workgroups with a partial one, two vertex workgroups"""
    s = _drape(N)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    ctx.set_param("contact", 0)
    NV = s.tot_NV
    assert NV == (N + 1) ** 2 and ctx.contact_counts() == (0, 0)
    xp, x = _moved(s.pos.to_numpy(), np.arange(NV), seed=N)
    tab = s.faces.to_numpy().reshape(-1, 3)
    assert len(tab) == 2 * N * N
    ids, w = _wind_list(np.arange(len(tab)), seed=N + 1)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    assert fz0.any()
    ctx.set_wind(ids, w)
    ctx.set_wind_velocity(W0)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [int(v) for v in tab[ids[w > 0]].reshape(-1) if not fz0[v].any()]
    _check_state(S, s, x, xp, tab, ids, w, [fz0, _frozen_pattern(fz0, touched)], s.cloths[0].NF)
    s._close_ctx()


def test_cloth_with_bodies_matches_the_restatement_and_body_faces_are_refused():
    """Scene_balancing with a 9 x 9-vertex cloth: bodies present, so the assembly takes the three-stream schedule (assemble_enqueue_early)"""
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=DX * 8, cloth_N=8, cloth_M=8)
    s.init_all()
    ctx = s._ensure_ctx()
    ctx.set_param("tet_warm", 0)   # (two assemblies of one state differ in the last bits of the bodies' blocks otherwise; the differences ask for exact zeros)
    ctx.set_param("contact", 0)
    cl = s.cloths[0]
    assert cl.NV == 81 and ctx.n_body > 1 and s.tot_NF > cl.NF
    NV = s.tot_NV
    cloth = np.arange(cl.offset, cl.offset + cl.NV)
    xp, x = _moved(s.pos.to_numpy(), cloth, seed=5)
    tab = s.faces.to_numpy().reshape(-1, 3)
    ids, w = _wind_list(cl.faces(), seed=6)
    fz0 = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_wind(ids, w)
    ctx.set_wind_velocity(W0)
    S = _State(ctx, x, xp, s._ref_angle)
    touched = [int(v) for v in tab[ids[w > 0]].reshape(-1) if not fz0[v].any()]
    _check_state(S, s, x, xp, tab, ids, w, [fz0, _frozen_pattern(fz0, touched)], cl.NF)
    # a surface face of a body: refused by the library and by the scene, the list stays
    pos = _dev(x)
    before = ctx.wind_force(pos, _dev(xp))
    body_face = int(cl.offset_faces + cl.NF)
    pat = r"face %d of entry 1 is a surface face of a body, not a cloth face \(cloth faces are \[0, %d\)\)" % (body_face, cl.NF)
    with pytest.raises(Exception, match="tsl_set_wind: " + pat):
        ctx.set_wind([3, body_face], None)
    with pytest.raises(ValueError, match="set_wind: " + pat):
        s.set_wind(1.0, 1.0, face_ids=[3, body_face])
    assert ctx.wind_count() == len(ids) and np.array_equal(ctx.wind_force(pos, _dev(xp)), before)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ degenerate face
def test_a_face_collapsed_at_the_start_of_the_step_contributes_exact_zeros():
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    ctx.set_param("contact", 0)
    NV = s.tot_NV
    xp, x = _moved(s.pos.to_numpy(), np.arange(NV), seed=3)
    tab = s.faces.to_numpy().reshape(-1, 3)
    ids, w = _wind_list(np.arange(len(tab)), seed=4)
    k = int(np.nonzero(w > 0)[0][5])
    f = tab[ids[k]]
    assert not s.frozen.to_numpy().reshape(-1, 3)[f].any()
    xp[f[2]] = xp[f[1]]                      # A0 = 0 in x_prev only
    assert np.abs(np.cross(x[f[1]] - x[f[0]], x[f[2]] - x[f[0]])).max() > 0
    fz = s.frozen.to_numpy().reshape(-1, 3)
    ctx.set_wind_velocity(W0)
    # the face alone: exact zeros everywhere
    ctx.set_wind(ids[k:k + 1], w[k:k + 1])
    S = _State(ctx, x, xp, s._ref_angle)
    assert S.part(S.energy) == 0.0 and not S.part(S.grad).any() and not S.part(lambda: S.operator(1)).any()
    p = _dev(np.random.default_rng(2).normal(size=3 * NV))
    assert np.array_equal(ctx.wind_force(S.pos, S.prev), np.zeros(3)) and np.array_equal(ctx.wind_grad(S.pos, S.prev, p), np.zeros(5))
    p2, share, wg = _reverse_step(S, NV, s.cloths[0].NF, s.mass.to_numpy(), s.dt, fz)
    assert np.abs(p2).max() > 0 and np.array_equal(wg, np.zeros(5))
    S.on(False)
    _, share0, _ = _reverse_step(S, NV, s.cloths[0].NF, s.mass.to_numpy(), s.dt, fz)
    assert np.array_equal(share, share0)
    # among the others: the restatement leaves it out, nothing is NaN
    ctx.set_wind(ids, w)
    args = (tab[ids], w, W0, CN, CT, s.dt)
    e, g = S.part(S.energy), S.part(S.grad)
    e_np, g_np = wn.energy(x, xp, *args), wn.gradient(x, xp, *args) * (fz == 0)
    assert np.isfinite(e) and np.isfinite(g).all() and abs(e - e_np) <= 1e-12 * abs(e_np) and np.abs(g - g_np).max() <= 1e-12 * np.abs(g_np).max()
    D = S.part(lambda: S.operator(0))
    assert np.isfinite(D).all()
    wg = ctx.wind_grad(S.pos, S.prev, p)
    wg_np = wn.wind_grad(x, xp, p.cpu().numpy().reshape(-1, 3), fz, *args)
    assert np.isfinite(wg).all() and np.abs(wg - wg_np).max() <= 1e-12 * np.abs(wg_np).max()
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


@pytest.mark.parametrize("how", ["removed", "coefficients_zero", "weights_zero"])
def test_off_means_off(how):
    """a context that had wind and lost it -- the list removed, both coefficients 0, every weight 0 -- gives the bits of one that never heard of wind:
    energy, gradient, operator and one step.  (The first two launch no wind kernel; the third adds exact zeros.)"""
    rng = np.random.default_rng(5)
    fresh = _drape(12, perturb=1e-4)
    x = fresh.pos.to_numpy()
    y = x + rng.normal(scale=1e-4, size=x.shape) * (fresh.frozen.to_numpy().reshape(-1, 3) == 0)
    ctx_f = fresh._ensure_ctx()
    ctx_f.set_param("direct", 1)
    want = _assemble_and_step(ctx_f, y, fresh._ref_angle)
    used = _drape(12, perturb=1e-4)
    used.set_wind(200.0, 20.0)
    used.set_wind_velocity([0.3, 0.2, 1.0])
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    st = used.time_step(None, 1)
    assert st["unconverged"] == 0 and ctx_u.wind_count() == 288 and np.abs(used.wind_force()).max() > 0
    assert not np.array_equal(_assemble_and_step(ctx_u, y, used._ref_angle)[0], want[0])
    if how == "removed":
        used.set_wind(0.0, 0.0, face_ids=[])
        assert used._ensure_ctx() is ctx_u and ctx_u.wind_count() == 0
    elif how == "coefficients_zero":
        ctx_u.set_param("wind_cn", 0.0); ctx_u.set_param("wind_ct", 0.0)
        f = ctx_u.wind_force(_dev(y), _dev(y))
        assert ctx_u.wind_count() == 288 and f.shape == (3,) and not f.any()
    else:
        used.set_wind(200.0, 20.0, weights=np.zeros(288))
        assert used._ensure_ctx() is ctx_u and ctx_u.wind_count() == 288
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, c in zip(want, got):
        assert np.array_equal(a, c)
    fresh._close_ctx(); used._close_ctx()


# ------------------------------------------------------------------------------------------------ momentum
def test_total_momentum_of_a_free_sheet():
    """A free sheet (no frozen dof, no contact) under gravity in a wind, one step from a moving start: the elastic forces cancel in the sum over the
    vertices, so  sum_v m_v (x_v - xp_v - dt vel_v) / dt^2 = sum_v m_v g_v + wind_force  per axis, a closed form independent of the restatement.
    The two sides differ by the sum of the rows of the step's final gradient F, at most sqrt(NV) |F|_2 per axis; the step's statistics report no
    gradient norm (last_delta is |p|max / dt), so |F|_2 is taken from one assembly at the converged state.  Bound: sqrt(NV) |F|_2 + 1e-12 of the
    largest term.  Measured (MI355X): gap 1.9e-14, 1.0e-14, 1.3e-15 N per axis against terms of 0.045, 0.091 and 2.9 N; |F|_2 = 1.0e-9, bound 1.3e-8 N."""
    s = _drape(12, pin=False, perturb=1e-4)
    NV = s.tot_NV
    assert not s.frozen.to_numpy().any()
    s.set_wind(200.0, 20.0)
    W = np.array([0.4, -0.7, 1.5])
    s.set_wind_velocity(W)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    ctx.set_param("contact", 0)
    rng = np.random.default_rng(9)
    x0 = s.pos.to_numpy()
    v0 = np.array([0.05, 0.02, -0.1]) + rng.normal(scale=1e-3, size=x0.shape)
    pos, prev, vel = _dev(x0), _dev(x0), _dev(v0)
    st = ctx.step(pos, prev, vel, s._ref_angle)
    assert st["unconverged"] == 0 and st["newton_iters"] < 50, st
    x1 = pos.cpu().numpy()
    assert np.array_equal(prev.cpu().numpy(), x0)
    m = s.mass.to_numpy()
    dt = s.dt
    lhs = (m[:, None] * (x1 - x0 - dt * v0)).sum(axis=0) / dt ** 2
    grav = (m[:, None] * s._gravity_array().reshape(-1, 3)).sum(axis=0)
    assert grav[2] < 0
    wf = ctx.wind_force(pos, prev)
    F = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, _dev(v0), s._ref_angle, spd=1, grad=F)
    fn = float(F.norm())
    big = max(np.abs(lhs).max(), np.abs(grav).max(), np.abs(wf).max())
    bound = np.sqrt(NV) * fn + 1e-12 * big
    print("momentum: lhs %s, gravity %s + wind %s; gap %s N, |F|_2 %.3e, bound %.3e, last_delta %.2e" % (lhs, grav, wf, np.abs(lhs - (grav + wf)), fn, bound, st["last_delta"]))
    assert np.abs(wf).min() > 1e-3 * np.abs(grav).max()
    assert np.abs(lhs - (grav + wf)).max() <= bound


# ------------------------------------------------------------------------------------------------ limits
def test_isotropic_limit_and_tangential_wind():
    """c_n = c_t = c with all weights 1: the block of every corner pair of a face is c A0 / (9 dt) I and a corner's gradient c A0 r / 3, summed over
    the faces.  W in the plane of a flat sheet at rest with c_t = 0: the gradient is exactly 0."""
    s = _drape(8)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    ctx.set_param("contact", 0)
    NV = s.tot_NV
    ctx.set_frozen(np.zeros(3 * NV, np.int32))
    x0 = s.pos.to_numpy()
    xp, x = _moved(x0, np.arange(NV), seed=12)
    tab = s.faces.to_numpy().reshape(-1, 3)
    ctx.set_wind(None, None)
    assert ctx.wind_count() == len(tab)
    ctx.set_wind_velocity(W0)
    c = 3.0e8
    S = _State(ctx, x, xp, s._ref_angle, cn=c, ct=c)
    g_cf = np.zeros((NV, 3)); H_cf = np.zeros((3 * NV, 3 * NV))
    for f in tab:
        A0 = 0.5 * np.linalg.norm(np.cross(xp[f[1]] - xp[f[0]], xp[f[2]] - xp[f[0]]))
        r = (x[f].mean(axis=0) - xp[f].mean(axis=0)) / s.dt - W0
        for a in f:
            g_cf[a] += c * A0 * r / 3.0
            for b in f:
                H_cf[3 * a:3 * a + 3, 3 * b:3 * b + 3] += c * A0 / (9.0 * s.dt) * np.eye(3)
    g, D = S.part(S.grad), S.part(lambda: S.operator(1))
    print("isotropic: gradient %.2e, operator %.2e of the largest entry" % (np.abs(g - g_cf).max() / np.abs(g_cf).max(), np.abs(D - H_cf).max() / np.abs(H_cf).max()))
    assert np.abs(g - g_cf).max() <= 1e-12 * np.abs(g_cf).max() and np.abs(D - H_cf).max() <= 1e-12 * np.abs(H_cf).max()
    off = ~np.kron(np.ones((NV, NV), bool), np.eye(3, dtype=bool))
    assert (D[off] == 0).all()                      # multiples of the identity
    # a flat sheet at rest, the wind in its plane, no tangential drag
    assert np.ptp(x0[:, 2]) == 0.0
    T = _State(ctx, x0, x0, s._ref_angle, cn=CN, ct=0.0)
    ctx.set_wind_velocity([0.4, -0.3, 0.0])
    gt = T.part(T.grad)
    assert np.array_equal(gt, np.zeros((NV, 3)))
    ctx.set_wind_velocity([0.4, -0.3, 0.1])
    assert np.abs(T.part(T.grad)[:, 2]).max() > 0 and not T.part(T.grad)[:, :2].any()
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ whole rollouts
STVK = (3.0e5, 2.0e5)
W_FLAG = np.array([0.3, 1.0, 0.1])


def _flag(**kw):
    from thinshelllab_amd.task_scene.Scene_flag import Scene
    s = Scene(**kw)
    s.init_all()
    s._ensure_ctx().set_param("direct", 1)
    return s


ROLLOUT_SCENE = dict(Kb=0.0, stvk=STVK, newton_cap=200, wind=(0.3, 3.0, 0.1))   # (relaxed in a wind of 3 m / s: the sheet is taut when the rollout starts)
RELAX_STEPS = 30
_RELAXED = {}


def _relaxed(scene, relax):
    """the rollout scene's start, computed once: the StVK flag without bending (its matrix is the exact second derivative of its energy), hung by two
    corners, after `relax` steps in the scene's wind (positions, velocities).  A sheet without bending stiffness that hangs slack wrinkles, and a
    wrinkle that flips under a perturbation of 1e-6 m makes the time stepper itself non-smooth: in the scene's default wind of 1 m / s the
    differences in x_0 scatter by their own size at every step from 1e-5 to 3e-8 m.  Relaxed in 3 m / s the drag keeps the sheet taut and the
    differences settle (DESIGN.md 2.13 has both tables)."""
    key = (repr(sorted(scene.items())), relax)
    if key not in _RELAXED:
        s = _flag(**scene)
        for f in range(1, relax + 1):
            assert s.time_step(None, f)["unconverged"] == 0
        _RELAXED[key] = (s.pos.to_numpy().copy(), s.vel.to_numpy().copy())
        s._close_ctx()
    return _RELAXED[key][0].copy(), _RELAXED[key][1].copy()


# The two difference steps of every check, a decade apart, chosen by measurement (every step from 1e-1 to 1e-3 m / s, 10 to 0.1 N s / m^3 and 1e-5 to
# 3e-8 m was run): the wind velocity against its own size of 1 m / s, the coefficients against theirs (200 and 20 N s / m^3).  The
# start positions move along white noise of unit size per dof: from 1e-6 m on that strains the membrane (3e5 N / m) enough to change the rollout
# beyond the linear range (differences of -5.4e-2, 1.8e-2, 5.38e-2 at 1e-6, 3e-6, 1e-5 m against 5.409e-2 below), so its steps are 3e-7 and 3e-8 m.
# The differences are those of the time stepper as it is: its Newton iteration stops at |p|max / dt < 1e-7, so they differentiate an iterate
# slightly off the stationary point that the reverse step assumes; steps this size keep the differences' own disagreement above that.
FD_STEPS = {"W": (1e-1, 1e-2), "cn": (1e1, 1e0), "ct": (1e1, 1e0), "x": (3e-7, 3e-8)}


def _rollout_setup(scene=ROLLOUT_SCENE, relax=RELAX_STEPS):
    """[(name, key of FD_STEPS, analytic value, h -> central difference at step h)] of the rollout, and the scene to close"""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    x0, v0 = _relaxed(scene, relax)
    s = _flag(**scene)
    cap = scene.get("newton_cap", 50)
    cn0, ct0 = s.wind_cn, s.wind_ct
    rng = np.random.default_rng(8)
    wgt = rng.normal(scale=1e-2, size=x0.shape)
    W_traj = W_FLAG[None] + np.array([[0.0, 0.0, 0.0], [0.1, -0.2, 0.05], [-0.1, 0.1, 0.2], [0.2, 0.3, -0.1]])
    free = (s.frozen.to_numpy().reshape(-1, 3) == 0)

    def rollout(W=W_traj, cn=cn0, ct=ct0, x=x0, reverse=False):
        s.set_wind(cn, ct)
        # (row 0 of the tape is d(loss)/d(x_0) with the state before it held fixed: the start velocity moves with the start state)
        s.pos.from_numpy(x); s.prev_pos.from_numpy(x); s.vel.from_numpy(v0 + (x - x0) * (s.damping / s.dt))
        g = Grad(s, T, 0); g.init_mass(s)
        g.count_kb_grad = False
        s.set_wind_velocity(W[0])
        g.copy_pos(s, 0)
        for fr in range(1, T):
            s.set_wind_velocity(W[fr])
            st = s.time_step(None, fr)
            assert st["unconverged"] == 0 and st["newton_iters"] < cap, st
            if reverse:
                print("step %d: %d Newton iterations, last delta %.2e" % (fr, st["newton_iters"], st["last_delta"]))
            g.copy_pos(s, fr)
        xs = g.pos_buffer.t.cpu().numpy()
        L = float((xs[T - 1] * wgt).sum())
        if not reverse:
            return L
        assert np.array_equal(g.wind_velocity.t.numpy(), W)
        g.pos_grad.t[T - 1] = _dev(wgt)
        for fr in range(T - 1, 0, -1):
            g.transfer_grad(fr, s, None)
            assert g.last_stats["flag"] != 3 and g.pos_grad.t[fr - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.wind_grad.t.numpy().copy(), g.wind_velocity_grad().numpy().copy(), g.pos_grad.t[0].cpu().numpy().copy()

    _, wg, vg, pg0 = rollout(reverse=True)
    assert wg.shape == (T, 5) and vg.shape == (T, 3) and (wg[0] == 0).all() and np.abs(wg[1:]).min() > 0 and np.array_equal(vg, wg[:, 0:3])
    d_W = rng.uniform(-1.0, 1.0, (T, 3))
    e = rng.normal(size=x0.shape) * free
    cd = lambda f: (lambda h: (f(h) - f(-h)) / (2 * h))
    return [("wind_velocity_grad . delta_W", "W", float((vg * d_W).sum()), cd(lambda h: rollout(W=W_traj + h * d_W))),
            ("sum_s wind_grad[s, 3] (c_n)", "cn", float(wg[:, 3].sum()), cd(lambda h: rollout(cn=cn0 + h))),
            ("sum_s wind_grad[s, 4] (c_t)", "ct", float(wg[:, 4].sum()), cd(lambda h: rollout(ct=ct0 + h))),
            ("pos_grad[0] . direction", "x", float((pg0 * e).sum()), cd(lambda h: rollout(x=x0 + h * e)))], s


def _rollout_checks(steps=FD_STEPS, scene=ROLLOUT_SCENE, relax=RELAX_STEPS):
    """[(name, analytic, (difference at the larger step, at the smaller step))]"""
    setup, s = _rollout_setup(scene, relax)
    checks = [(name, got, [f(h) for h in steps[key]]) for name, key, got, f in setup]
    for name, got, d in checks:
        print("%s: analytic %.10e, differences %s" % (name, got, " / ".join("%.10e" % v for v in d)))
        print("    (the last two disagree %.2e relative), error %.2e relative, bound %.2e relative"
              % (abs(d[-2] - d[-1]) / abs(d[-1]), abs(got - d[-1]) / abs(d[-1]), 3 * abs(d[-2] - d[-1]) / abs(d[-1])))
    s._close_ctx()
    return checks


def test_whole_rollout_gradients_match_differences():
    """T = 4, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2, asserted), a random linear loss on the last state; Scene_flag
    with the StVK sheet without bending, relaxed for 30 steps in a wind of 3 m / s; the wind velocity (about 1 m / s) then changes from step to step.
    wind_velocity_grad() contracted with a random (T, 3) direction, the c_n and c_t columns summed over the steps, and pos_grad[0] . e along a random
    free direction (the state before it held fixed), each against central differences at two steps a decade apart.  Rule of
    test_gpu_spheres.py::test_whole_rollout_gradients_match_differences: the two differences agree to 1e-2 of the value, and the analytic value
    lies within three times their disagreement.  Measured at FD_STEPS (MI355X): errors 8.6e-6, 5.1e-6, 2.1e-6 and 2.5e-5 relative against bounds
    of 4.3e-4, 3.1e-5, 2.3e-4 and 3.6e-4; the two differences disagree by 1.4e-4, 1.0e-5, 7.7e-5 and 1.2e-4."""
    for name, got, fd in _rollout_checks():
        assert abs(fd[0] - fd[1]) < 1e-2 * abs(fd[1]), name
        assert abs(got - fd[1]) <= 3 * abs(fd[0] - fd[1]), name


# ------------------------------------------------------------------------------------------------ groups and plans
T_TAPE = 5


def _tape(s):
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    g = Grad(s, T_TAPE, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    return g


def _blown(W, dW):
    s = _flag(N=8)
    return s, (lambda f: np.asarray(W) + np.asarray(dW) * f)


def test_group_members_equal_their_single_runs_and_two_runs_repeat():
    from thinshelllab_amd.scene_group import SceneGroup
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(81, 3))
    A, B = ((0.3, 1.0, 0.1), (0.05, 0.1, 0.0)), ((-0.5, 0.4, 0.3), (0.0, -0.1, 0.05))
    runs = {}
    for tag, wind in (("a", A), ("b", A), ("c", B)):
        s, W_of = _blown(*wind)
        g = _tape(s)
        for f in range(1, T_TAPE):
            s.set_wind_velocity(W_of(f))
            st = s.time_step(None, f)
            assert st["unconverged"] == 0 and st["factorizations"] > 0, st
            g.copy_pos(s, f)
        g.pos_grad.t[T_TAPE - 1] = _dev(wgt)
        for f in range(T_TAPE - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.last_stats["flag"] != 3
        runs[tag] = (g.pos_buffer.t.cpu().numpy().copy(), g.pos_grad.t.cpu().numpy().copy(), g.wind_grad.t.numpy().copy(), g.wind_velocity.t.numpy().copy())
        s._close_ctx()
    for a, b in zip(runs["a"], runs["b"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(runs["a"][0], runs["c"][0]) and np.abs(runs["a"][2][1:]).min() > 0 and (runs["a"][2][0] == 0).all()
    members = [_blown(*A), _blown(*B)]
    ms = [m[0] for m in members]
    G = SceneGroup(ms)
    gs = [_tape(m) for m in ms]
    for f in range(1, T_TAPE):
        for m, W_of in members:
            m.set_wind_velocity(W_of(f))
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
        assert np.array_equal(gs[i].wind_grad.t.numpy(), runs[tag][2]) and np.array_equal(gs[i].wind_velocity.t.numpy(), runs[tag][3]), i
    for m in ms:
        m._close_ctx()


def test_wind_builds_no_plan_and_no_slot():
    """the factorised path: the plan count after the first step does not change when the wind is switched on, over the rollout or in the reverse sweep"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    T = 4
    s = _flag(N=8)
    s.set_wind(0.0, 0.0, face_ids=[])
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    st = s.time_step(None, 1)
    assert st["unconverged"] == 0 and st["factorizations"] > 0 and ctx.wind_count() == 0
    plans = ctx.direct_info()["plans"]
    assert plans >= 1
    s.set_wind(200.0, 20.0)
    g = Grad(s, T, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    for f in range(1, T):
        s.set_wind_velocity([0.3, 1.0 + 0.1 * f, 0.1])
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["factorizations"] > 0 and st["nc"] == 0, st
        g.copy_pos(s, f)
        assert ctx.direct_info()["plans"] == plans and ctx.contact_counts() == (0, 0) and len(ctx.constraints()["idx"]) == 0
    assert s._ensure_ctx() is ctx and ctx.wind_count() == 128 and np.abs(s.wind_force()).max() > 0
    g.pos_grad.t[T - 1] = _dev(np.random.default_rng(7).normal(scale=1e-2, size=(s.tot_NV, 3)))
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3
    assert ctx.direct_info()["plans"] == plans and np.abs(g.wind_grad.t.numpy()[1:]).max() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_name_the_offender_and_keep_the_previous_list():
    s = _flag(N=8)
    ctx = s._ensure_ctx()
    ctx.set_wind([5, 3, 100], [1.0, 0.5, 2.0])
    pos = _dev(s.pos.to_numpy())
    before = ctx.wind_force(pos, pos)
    assert before.shape == (3,) and np.abs(before).max() > 0
    cases = [(([3, 7, 3], None), r"face 3 is listed twice \(entries 0 and 2\)"),
             (([3, 128], None), r"face 128 of entry 1 out of range \[0, 128\)"),
             (([3, -2], None), r"face -2 of entry 1 out of range \[0, 128\)"),
             (([3, 7], [1.0, -0.5]), r"weight -0.5 of entry 1 \(face 7\) is negative or not finite"),
             (([3, 7], [np.nan, 1.0]), r"weight nan of entry 0 \(face 3\) is negative or not finite")]
    for (f, w), pat in cases:
        with pytest.raises(Exception, match="tsl_set_wind: " + pat):
            ctx.set_wind(f, w)
        with pytest.raises(ValueError, match="set_wind: " + pat):          # the scene's host check: the library's message
            s.set_wind(1.0, 1.0, face_ids=f, weights=w)
        assert ctx.wind_count() == 3 and np.array_equal(ctx.wind_force(pos, pos), before)
    with pytest.raises(Exception, match=r"tsl_set_wind_velocity: component 1 of the wind velocity \(0, inf, 1\) is not finite"):
        ctx.set_wind_velocity([0.0, np.inf, 1.0])
    with pytest.raises(Exception, match=r"tsl_set_wind_velocity: component 2 of the wind velocity \(0, 0, nan\) is not finite"):
        ctx.set_wind_velocity([0.0, 0.0, np.nan])
    for key in ("wind_cn", "wind_ct"):
        with pytest.raises(Exception, match=key + " must be finite and >= 0"):
            ctx.set_param(key, -1.0)
        with pytest.raises(Exception, match=key + " must be finite and >= 0"):
            ctx.set_param(key, np.nan)
    assert ctx.wind_count() == 3 and np.array_equal(ctx.wind_force(pos, pos), before)
    # every cloth face: faces None
    ctx.set_wind(None, None)
    assert ctx.wind_count() == 128
    ctx.set_wind([], None)
    assert ctx.wind_count() == 0 and not ctx.wind_force(pos, pos).any()
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_wind import optimise
    losses, W = optimise(N=8, T=4, iters=4, log=print)
    assert len(losses) == 4 and losses[-1] < losses[0] and min(losses[1:]) < losses[0], losses
    assert tuple(W.shape) == (4, 3) and (W[1:] != W[0]).any()
