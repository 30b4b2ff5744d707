"""Soft handles (tsl_set_handles, "k_handle"; csrc/k_handle.hpp): target springs on vertices.  The reference has no such term, so it
is checked against the NumPy restatement (tests/handle_numpy.py), finite differences, a closed form and whole-rollout differences.  Every handle
quantity of a state is taken as a difference against the same state with k_handle = 0: no handle kernel runs there and the rest of the energy,
gradient and matrix is formed by the same launches in both."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_numpy as hn  # noqa: E402

pytestmark = pytest.mark.gpu

# N/m, for the per-state checks: the size of the cloth's own diagonal entries (springs: 2 Kl / l ~ 3e5), so that a difference of two assembled
# matrices, each rounded at its own size, still holds the handle term to the 12 digits asked for
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

    def handle_part(self, fun, k=K):
        """fun() with k_handle = k minus fun() with k_handle = 0"""
        self.ctx.set_param("k_handle", k)
        a = fun()
        self.ctx.set_param("k_handle", 0.0)
        b = fun()
        self.ctx.set_param("k_handle", k)
        return a - b


def _case(name):
    """(scene, x, v, w, t): a perturbed gravity-free cloth with handles; 'sparse' = 4 corners + one interior vertex, unequal weights, one of them 0"""
    N = 16 if name == "N16_all" else 12
    s = _cloth(N)
    s._ensure_ctx().set_gravity(np.zeros((s.tot_NV, 3)))
    rng = np.random.default_rng({"N12_all": 1, "N16_all": 2, "sparse": 3}[name])
    dx = s.cloths[0].dx
    x = s.pos.to_numpy() + rng.normal(scale=0.15 * dx, size=(s.tot_NV, 3))
    if name == "sparse":
        v = np.array(s.cloths[0].corner_ids() + [5 * (N + 1) + 7], np.int32)
        w = np.array([1.0, 0.5, 2.0, 0.0, 1.5])
    else:
        v = rng.permutation(s.tot_NV).astype(np.int32)   # every vertex, in no particular order: 169 / 289 handles (a partial wave, two workgroups at 289)
        w = rng.uniform(0.25, 2.0, len(v))
    t = x[v] + rng.normal(scale=0.5 * dx, size=(len(v), 3))
    s.set_handles(v, K, w)
    s.set_handle_targets(t)
    return s, x, v, w, t


def _frozen_pattern(NV, v):
    fz = np.zeros((NV, 3), np.int32)
    fz[v[0]] = 1           # a handled vertex, all three dofs
    fz[v[1], 1] = 1        # a handled vertex, one dof
    fz[v[2], 0] = 1; fz[v[2], 2] = 1
    return fz


# ------------------------------------------------------------------------------------------------ 1. / 2. per state
def _check_state(S, x, v, w, t, frozen, rest_is_exact):
    """the per-state checks against the restatement at the state S (a _State whose context holds the handles (v, w, t) with k_handle = K).
    rest_is_exact: nothing but the mass diagonal shares the matrix entries of the handles (the cloth's stiffnesses are zero), so the rest cancels
    bit for bit in the difference and the three spd modes must give the same bits.  With element blocks in place every assembled entry is rounded
    after the blocks of its mode were added -- fl(fl(m / dt^2 + k w) + S_spd) - fl(m / dt^2 + S_spd) -- and the last bit of the difference follows
    S_spd: there the modes are held to the restatement within the bound, each of them, and the number of entries that differ is printed."""
    NV = len(x)
    fzb = frozen.astype(bool)
    e = S.handle_part(S.energy)
    e_np = hn.energy(x, v, w, t, K)
    print("energy %.17g restatement %.17g rel %.2e" % (e, e_np, abs(e - e_np) / abs(e_np)))
    assert abs(e - e_np) <= 1e-12 * abs(e_np)
    g = S.handle_part(S.grad)
    g_np = hn.gradient(x, v, w, t, K, frozen)
    print("gradient err / max %.2e" % (np.abs(g - g_np).max() / np.abs(g_np).max()))
    assert np.abs(g - g_np).max() <= 1e-12 * np.abs(g_np).max()
    assert (g[fzb] == 0).all()
    D = [S.handle_part(lambda spd=spd: S.matrix(spd)) for spd in (0, 1, 2)]
    d_np = hn.diagonal(NV, v, w, K, frozen).ravel()
    off = D[0] - np.diag(np.diag(D[0]))
    print("matrix: diagonal err / k w max %.2e, off-diagonal max %.2e, entries where spd 1 / spd 2 differ from spd 0: %d / %d (max %.2e / %.2e)"
          % (np.abs(np.diag(D[0]) - d_np).max() / d_np.max(), np.abs(off).max(), (D[1] != D[0]).sum(), (D[2] != D[0]).sum(),
             np.abs(D[1] - D[0]).max(), np.abs(D[2] - D[0]).max()))
    if rest_is_exact:
        assert np.array_equal(D[0], D[1]) and np.array_equal(D[0], D[2])
    for Dm in D:
        assert (Dm - np.diag(np.diag(Dm)) == 0).all()
        assert np.abs(np.diag(Dm) - d_np).max() <= 1e-12 * d_np.max()
        assert (np.diag(Dm)[fzb.ravel()] == 0).all()


@pytest.mark.parametrize("name", ["N12_all", "N16_all", "sparse"])
def test_energy_gradient_and_matrix_match_the_restatement(name):
    s, x, v, w, t = _case(name)
    S = _State(s, x)
    NV = s.tot_NV
    free, fz = np.zeros((NV, 3), np.int32), _frozen_pattern(NV, v)
    for exact in (False, True):   # the cloth as it is, then with its stiffnesses at zero: only the mass diagonal under the handle entries
        if exact:
            for k in ("Kl", "Ka", "Kb"):
                S.ctx.set_param("cloth0." + k, 0.0)
        for frozen in (free, fz):
            S.ctx.set_frozen(frozen.reshape(-1))
            _check_state(S, x, v, w, t, frozen, exact)
    s._close_ctx()


@pytest.mark.parametrize("name", ["N12_all", "N16_all", "sparse"])
def test_force_target_gradient_and_stiffness_key(name):
    s, x, v, w, t = _case(name)
    S = _State(s, x)
    ctx, NV = S.ctx, s.tot_NV
    fz = _frozen_pattern(NV, v)
    ctx.set_frozen(fz.reshape(-1))
    f = ctx.handle_force(S.pos)
    f_np = hn.force(x, v, w, t, K)
    assert np.abs(f - f_np).max() <= 1e-14 * np.abs(f_np).max()
    assert (f[0] != 0).all()   # (frozen dofs are not masked in the read-out)
    pn = np.random.default_rng(11).normal(size=3 * NV)
    p = _dev(pn)
    tg = ctx.handle_grad(p)
    tg_np = hn.target_grad(pn, v, w, K, fz)
    assert np.abs(tg - tg_np).max() <= 1e-14 * np.abs(tg_np).max()
    assert (tg[0] == 0).all() and tg[1, 1] == 0 and tg[2, 0] == 0 and tg[2, 2] == 0 and tg[1, 0] != 0
    # the k_handle key against central differences of the assembled (masked) gradient: the term is linear in k_handle
    got = ctx.param_grads(S.pos, S.ref, ["k_handle"], p=p)["k_handle"]
    h = 0.5 * K
    ctx.set_param("k_handle", K + h); gp = S.grad()
    ctx.set_param("k_handle", K - h); gm = S.grad()
    ctx.set_param("k_handle", K)
    fd = -float(np.dot(pn, (gp - gm).ravel() / (2 * h)))
    print("k_handle key %.15g differences %.15g restatement %.15g" % (got, fd, hn.k_deriv(x, pn, v, w, t, fz)))
    assert abs(got - fd) <= 1e-8 * abs(fd)
    # existing keys keep their bits when k_handle is asked too, and k_handle keeps its own
    old = ["cloth0.Kl", "cloth0.Ka", "cloth0.Kb"]
    a = ctx.param_grads(S.pos, S.ref, old, p=p)
    b = ctx.param_grads(S.pos, S.ref, ["k_handle"] + old[:2] + ["k_handle"] + old[2:], p=p)
    assert all(a[k] == b[k] for k in old) and b["k_handle"] == got
    s._close_ctx()


def test_k_handle_key_is_zero_without_handles_and_errors_name_the_offender():
    from thinshelllab_amd._lib import TslError
    s = _cloth(12)
    ctx = s._ensure_ctx()
    S = _State(s, s.pos.to_numpy())
    p = _dev(np.random.default_rng(0).normal(size=3 * s.tot_NV))
    assert ctx.param_grads(S.pos, S.ref, ["k_handle"], p=p)["k_handle"] == 0.0
    with pytest.raises(TslError, match="vertex 7 has more than one handle"):
        ctx.set_handles([3, 7, 7])
    with pytest.raises(TslError, match=r"vertex 169 out of range \[0, 169\)"):
        ctx.set_handles([169])
    with pytest.raises(TslError, match="weight -1 of vertex 4 is negative or not finite"):
        ctx.set_handles([2, 4], [1.0, -1.0])
    with pytest.raises(TslError, match="k_handle"):
        ctx.set_param("k_handle", -1.0)
    assert ctx.handle_force(S.pos).shape == (0, 3)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ 3. closed form
@pytest.mark.parametrize("direct", [1, 0])
def test_one_step_towards_translated_targets_has_a_closed_form(direct):
    """every vertex handled with weight 1, the cloth at rest, targets = rest + d: internal forces vanish under a translation, so one implicit step
    solves (m / dt^2 + k) (x - x0) = k d per vertex.  Bound: 100 cg_tol |d| -- the linear solve's own tolerance with a margin for the Newton stop."""
    s = _cloth(12)
    ctx = s._ensure_ctx()
    ctx.set_gravity(np.zeros((s.tot_NV, 3)))
    for k, val in (("damping", 0.0), ("cg_tol", 1e-10), ("direct", direct)):
        ctx.set_param(k, val)
    x0 = s.pos.to_numpy()
    dx = s.cloths[0].dx
    d = dx * np.array([2.0, -1.0, 2.0]) / 3.0
    k = 300.0
    s.set_handles(np.arange(s.tot_NV), k)
    s.set_handle_targets(x0 + d)
    st = s.time_step(None, 1)
    m = s.mass.to_numpy()[:, None]
    want = x0 + d * k / (k + m / s.dt ** 2)
    err = np.abs(s.pos.to_numpy() - want).max()
    print("closed form, direct = %d: max error %.3e m (bound %.3e), Newton iterations %d, solves %d" % (direct, err, 100 * 1e-10 * dx, st["newton_iters"], st["solves"]))
    assert st["unconverged"] == 0
    assert (st["factorizations"] > 0) == (direct == 1)
    assert err <= 100 * 1e-10 * np.linalg.norm(d)
    f = s.handle_force()
    assert np.abs(f - k * (x0 + d - s.pos.to_numpy())).max() <= 1e-12 * np.abs(f).max()
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ 4. off means off
def _assemble_and_step(ctx, x, ref):
    pos = _dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, ref, spd=1, grad=F)
    H = ctx.matrix()[2].copy()
    e = ctx.energy(pos, prev, vel, ref)
    ctx.set_param("contact", 0.0)
    st = ctx.step(pos, prev, vel, ref)
    return F.cpu().numpy(), H, e, pos.cpu().numpy(), vel.cpu().numpy(), st["newton_iters"]


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
    used.set_handles(used.cloths[0].corner_ids()[:2], K, [1.0, 2.0])
    used.set_handle_targets(x[used.cloths[0].corner_ids()[:2]] + 1e-3)
    ctx_u = used._ensure_ctx()
    ctx_u.set_param("direct", 1)
    plans = []
    st = used.time_step(None, 1)
    plans.append(ctx_u.direct_info()["plans"])
    assert st["unconverged"] == 0 and np.abs(used.handle_force()).max() > 0
    if how == "removed":
        used.set_handles([], 0.0)
        assert used._ensure_ctx() is ctx_u
    else:
        ctx_u.set_param("k_handle", 0.0)
    got = _assemble_and_step(ctx_u, y, used._ref_angle)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    # the plans of the factorisation do not depend on handles: none is built when handles are added or moved
    used.set_handles(used.cloths[0].corner_ids(), K)
    used.set_handle_targets(x[used.cloths[0].corner_ids()])
    used.time_step(None, 2)
    plans.append(used._ensure_ctx().direct_info()["plans"])
    used.set_handle_targets(x[used.cloths[0].corner_ids()] + 2e-3)
    used.time_step(None, 3)
    plans.append(used._ensure_ctx().direct_info()["plans"])
    assert plans[0] >= 1 and plans[1] == plans[0] and plans[2] == plans[0], plans
    fresh._close_ctx(); used._close_ctx()


# ------------------------------------------------------------------------------------------------ 5.-7. the drape pinned by handles
# The sheet is the one of the StVK rollout checks (tests/test_gpu_stvk.py): membrane = 1, Kb = 0, flat from rest.  Its matrix is the exact second
# derivative of its energy, so whole-rollout gradients can be held to differences; the spring cloth's adjoint solves with the reference's own
# Hessian (factor 2 in the area block, slot-indexed bending terms: DESIGN.md 2.2), which is 1e-2 to 0.7 away from differences on a drape -- the
# handle gradients of a spring drape were 9e-3 (targets) and 1.6e-3 (k_handle) from differences when this test was written.
KD = 2000.0   # N/m: the 16 x 16 sheet weighs 5 N; two handles hold it with ~1 mm of stretch each
T_TAPE = 6


def _drape(direct=1, handles=True, cg_tol=None):
    """16 x 16 drape, gravity on; handles=True: the two corners of grid row N on handles instead of the pinned row"""
    s = _cloth(16, pin=not handles, perturb=0.0, Kb=0.0, stvk=(3.0e5, 2.0e5))
    if handles:
        s.set_handles(s.cloths[0].corner_ids()[2:], KD)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", direct)
    if cg_tol:
        ctx.set_param("cg_tol", cg_tol)
    return s


def _moving_targets(s, T, scale=1.0):
    x0 = s.pos.to_numpy()[s.cloths[0].corner_ids()[2:]]
    f = np.arange(T)[:, None, None]
    u = (x0[1] - x0[0]) / np.linalg.norm(x0[1] - x0[0])
    out = np.cross(u, [0.0, 0.0, 1.0])
    up = np.array([0.0, 0.0, 1.0])
    # per step: up and apart (a membrane without bending stiffness buckles under compression), the two handles differently
    move = scale * np.array([-1e-4 * u + 3e-4 * up + 1e-4 * out, 2e-4 * u + 2e-4 * up])
    return x0[None] + f * move[None]


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


def test_drape_on_handles_repeats_and_group_members_equal_their_single_runs():
    T = T_TAPE
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(289, 3))
    runs = []
    for scale in (1.0, 1.0, 0.5):
        s = _drape()
        g, st = _tape(s, _moving_targets(s, T, scale))
        assert all(r["factorizations"] > 0 for r in st)
        _reverse(s, g, wgt, T)
        runs.append((g.pos_buffer.t.cpu().numpy().copy(), g.handle_grad.t.numpy().copy()))
        s._close_ctx()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.abs(runs[0][0][-1] - runs[0][0][0]).max() > 1e-4 and np.abs(runs[0][1][1:]).min() > 0 and not np.array_equal(runs[0][0], runs[2][0])
    # S = 2, the members on different targets
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


def test_whole_rollout_gradients_match_differences():
    """T = 4 on the handle-pinned drape, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last
    state.  handle_grad[s] for every step and handled dof and grad_params["k_handle"] against central differences of the loss over whole rollouts
    at two step sizes a decade apart; the bound is ten times the disagreement of the two differences, and never looser than 1e-3 of the largest entry."""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    T = 4
    s = _drape(cg_tol=1e-13)
    x0 = s.pos.to_numpy()
    tg0 = _moving_targets(s, T)
    wgt = np.random.default_rng(8).normal(scale=1e-2, size=x0.shape)

    def rollout(targets, k=KD, reverse=False, tamper=None):
        _reset(s, x0)
        s._ensure_ctx().set_param("k_handle", k)
        g = Grad(s, T, 0); g.init_mass(s)
        g.param_keys = ["k_handle"]
        st = _forward(s, g, targets, T)
        assert all(r["unconverged"] == 0 and r["newton_iters"] < 200 for r in st)
        L = float((g.pos_buffer.t[T - 1].cpu().numpy() * wgt).sum())
        if not reverse:
            return L
        if tamper is not None:
            g.handle_targets.t[:] = torch.as_tensor(tamper)
        g.pos_grad.t[T - 1] = _dev(wgt)
        for f in range(T - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.pos_grad.t[f - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.handle_grad.t.numpy().copy(), g.grad_params["k_handle"]

    _, hg, gk = rollout(tg0, reverse=True)

    def cd_target(f, i, a, h):
        tp = tg0.copy(); tp[f, i, a] += h
        tm = tg0.copy(); tm[f, i, a] -= h
        return (rollout(tp) - rollout(tm)) / (2 * h)

    fd = np.zeros((2,) + hg.shape)
    for n, h in enumerate((1e-4, 1e-5)):
        for f in range(1, T):
            for i in range(2):
                for a in range(3):
                    fd[n, f, i, a] = cd_target(f, i, a, h)
    big = np.abs(fd[1]).max()
    disagree = np.abs(fd[0] - fd[1]).max()
    err = np.abs(hg - fd[1]).max()
    bound = min(10 * disagree, 1e-3 * big)
    print("handle_grad: max |entry| %.4e, differences at h = 1e-4 / 1e-5 disagree by %.2e (%.2e relative), analytic - difference %.2e (%.2e relative), bound %.2e"
          % (big, disagree, disagree / big, err, err / big, bound))
    fk = [(rollout(tg0, KD * (1 + r)) - rollout(tg0, KD * (1 - r))) / (2 * r * KD) for r in (2e-2, 2e-3)]
    bound_k = min(10 * abs(fk[0] - fk[1]), 1e-3 * abs(fk[1]))
    print("k_handle: analytic %.8e, differences at 2e-2 / 2e-3 of the value %.8e / %.8e (disagree %.2e relative), error %.2e relative, bound %.2e relative"
          % (gk, fk[0], fk[1], abs(fk[0] - fk[1]) / abs(fk[1]), abs(gk - fk[1]) / abs(fk[1]), bound_k / abs(fk[1])))
    assert (hg[0] == 0).all()
    assert err <= bound
    assert abs(gk - fk[1]) <= bound_k
    # the reverse pass used the targets of its own step: a tape whose targets are constant in time gives another handle_grad, and the k_handle
    # gradient of a reverse pass over the right states but targets pushed one step late differs from the right one
    _, hg_c, gk_c = rollout(np.repeat(tg0[:1], T, axis=0), reverse=True)
    assert not np.array_equal(hg_c, hg) and gk_c != gk
    _, hg_t, gk_t = rollout(tg0, reverse=True, tamper=np.concatenate([tg0[:1], tg0[:-1]]))
    assert np.array_equal(hg_t, hg)          # (k w p does not read the targets)
    assert abs(gk_t - gk) > 1e-2 * abs(gk)   # (the key does)
    s._close_ctx()


def test_iterative_hierarchy_agrees_with_the_factorised_path():
    """the tape of the handle-pinned drape with direct = 0 against direct = 1; the yardstick is the same comparison on the drape pinned by its frozen
    row (no handles: the behaviour before handles existed), ten times of which is allowed"""
    out = {}
    for handles in (False, True):
        xs = []
        for direct in (1, 0):
            s = _drape(direct=direct, handles=handles)
            g, st = _tape(s, _moving_targets(s, T_TAPE) if handles else None)
            xs.append(g.pos_buffer.t.cpu().numpy().copy())
            s._close_ctx()
        out[handles] = np.abs(xs[0] - xs[1]).max()
    print("max |x_direct - x_iterative| over the tape: pinned row %.3e m, handles %.3e m" % (out[False], out[True]))
    assert out[True] <= 10 * out[False]


# ------------------------------------------------------------------------------------------------ 8. contact
def test_handles_next_to_contact_constraints():
    """Scene_balancing (cloth on the ball between the tactile pads, the contact scene of tests/test_gpu_param_grad.py): a handle on a cloth vertex
    that is in contact and one on a free one; the per-state checks with constraints present (the three-stream assembly), then one forward and
    one reverse step"""
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
    for f in range(1, 3):
        s.action(f, dpos, drot)
        s.time_step(projection_query, f)
    ctx = s._ensure_ctx()
    pos, prev, vel, ref = s._state()
    ctx.contact_detect(prev, prev)
    cons = ctx.constraints()
    c = s.cloths[0]
    idx = cons["idx"]
    in_contact = np.unique(idx[(idx >= c.offset) & (idx < c.offset + c.NV)])
    assert len(cons["idx"]) > 0 and len(in_contact) > 0
    free = [u for u in c.corner_ids() if u not in set(in_contact.tolist())]
    v = np.array([int(in_contact[0]), int(in_contact[-1]), free[0]], np.int32)
    w = np.array([1.0, 0.5, 2.0])
    x = pos.cpu().numpy()
    t = x[v] + np.array([[2e-3, -1e-3, 2e-3], [-1e-3, 1e-3, 2e-3], [1e-3, 2e-3, -2e-3]])
    s.set_handles(v, K, w)
    s.set_handle_targets(t)
    assert s._ensure_ctx() is ctx
    S = _State(s, x)
    S.prev = prev.clone(); S.vel = vel.clone(); S.ref = ref
    fz = s.frozen.to_numpy().reshape(-1, 3)
    assert not fz[v].any()
    # (the eigen-clamp of the bodies' element blocks starts from the eigenvectors of the previous assembly, "tet_warm": two assemblies of one
    # state differ in the last bits of the bodies' blocks.  Off for the differences, which ask for exact zeros away from the handles.)
    ctx.set_param("tet_warm", 0)
    _check_state(S, x, v, w, t, fz, False)
    ctx.set_param("tet_warm", 1)
    f_h = ctx.handle_force(S.pos)
    assert np.abs(f_h - hn.force(x, v, w, t, K)).max() <= 1e-14 * np.abs(f_h).max()
    pn = np.random.default_rng(12).normal(size=3 * s.tot_NV)
    p = _dev(pn)
    tg = ctx.handle_grad(p)
    assert np.abs(tg - hn.target_grad(pn, v, w, K, fz)).max() <= 1e-14 * np.abs(tg).max()
    got = ctx.param_grads(S.pos, S.ref, ["k_handle"], p=p)["k_handle"]
    h = 0.5 * K
    ctx.set_param("k_handle", K + h); gp = S.grad()
    ctx.set_param("k_handle", K - h); gm = S.grad()
    ctx.set_param("k_handle", K)
    fd = -float(np.dot(pn, (gp - gm).ravel() / (2 * h)))
    assert abs(got - fd) <= 1e-8 * abs(fd)
    # one forward and one reverse step with the handles on (a softer spring and nearer targets: a pull the step can follow)
    s.set_handles(v, 500.0, w)
    s.set_handle_targets(x[v] + 0.1 * (t - x[v]))
    g = Grad(s, 2, n_part); g.init_mass(s)
    g.copy_pos(s, 0)
    s.action(3, dpos, drot)
    st = s.time_step(projection_query, 3)
    assert st["unconverged"] == 0 and st["nc"] > 0
    g.copy_pos(s, 1)
    g.pos_grad.t[1] = _dev(np.random.default_rng(13).normal(scale=1e-2, size=(s.tot_NV, 3)))
    g.transfer_grad(1, s, projection_query)
    assert g.last_stats["flag"] != 3 and np.abs(g.handle_grad.t[1].numpy()).max() > 0
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ 9. driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_handles import optimise
    losses, targets = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
