"""Parameter gradients by key (tsl_param_grad_keys, TslContext.param_grads, Grad.param_keys / grad_params): the vector-Jacobian product
p . d(force)/d(theta) of every material and contact scalar, checked without the oracle -- against central differences of tsl_assemble's
gradient at a fixed state and constraint set (every supported key enters it linearly: exact up to rounding), against the reference's own
tsl_param_grad / tsl_friction_grad, and against central differences of a loss over whole rollouts."""
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ee_numpy as en  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ scenes
def _task_scene(name):
    from thinshelllab_amd.engine.geometry import projection_query
    if name == "drape":
        from thinshelllab_amd.task_scene.Scene_drape import Scene
        s = Scene(cloth_size=0.1 / 15 * 12, N=12, M=12, Kb=100.0, k_angle=3.14, perturb=2e-3)
        s.init_all()
        for f in range(1, 3):
            s.time_step(None, f)
        return s
    if name == "balancing":
        from thinshelllab_amd.task_scene.Scene_balancing import Scene
        s = Scene(cloth_size=0.06)
        s.init_all()
        s.mu_cloth_elastic[None] = 5.0
    elif name == "bouncing":
        from thinshelllab_amd.task_scene.Scene_bouncing import Scene
        s = Scene(cloth_size=0.06)
        s.cloths[0].Kb[None] = 1400.0
        s.init_all()
        s.mu_cloth_elastic[None] = 0.5
    else:
        from thinshelllab_amd.task_scene.Scene_sliding import Scene
        s = Scene(cloth_size=0.06)
        s.cloths[0].Kb[None] = 1000.0
        s.mu_cloth_cloth[None] = 0.7
        s.init_all()
        s.mu_cloth_elastic[None] = 1.0
    s.prev_pos.copy_from(s.pos)
    x = s.pos.to_numpy()
    for k, c in enumerate(s.cloths):   # off the exact contact threshold (sheets lie eps_contact apart)
        x[c.offset:c.offset + c.NV, 2] += 2e-6 * np.sin(0.7 * np.arange(c.NV) + 0.3 + k) - 3e-6 * k
    s.pos.from_numpy(x); s.prev_pos.from_numpy(x)
    n_part = s.gripper.n_part if hasattr(s, "gripper") else 0
    dpos = np.zeros((n_part, 3)); drot = np.zeros((n_part, 3))
    dpos[:, 2] = 5e-5 if name == "balancing" else -1e-4
    dpos[:, 0] = 2e-4
    drot[:, 1] = 2e-3
    for f in range(1, 2 if name == "sliding" else 3):   # (the sheets of Scene_sliding push each other out of the contact shell soon)
        if n_part:
            s.action(f, dpos, drot)
        s.time_step(projection_query, f)
    return s


def _keys_and_values(s):
    kv = {}
    for i, c in enumerate(s.cloths):
        kv[f"cloth{i}.Kl"] = c.Kl.value; kv[f"cloth{i}.Ka"] = c.Ka.value; kv[f"cloth{i}.Kb"] = c.Kb.value
    for i, e in enumerate(s.elastics):
        kv[f"elastic{i}.mu"] = e.mu.value; kv[f"elastic{i}.lam"] = e.lam.value
    if s.elastics:
        kv["k_contact"] = float(s.k_contact)
        kv["mu_cloth_elastic"] = s.mu_cloth_elastic.value
        if hasattr(s, "mu_cloth_cloth"):
            kv["mu_cloth_cloth"] = s.mu_cloth_cloth.value
    return kv


def _grad_at(ctx, state, flag, dr, key, value):
    """tsl_assemble's gradient with `key` = value, the constraints detected again from the same positions and projection state"""
    pos, prev, vel, ref = state
    ctx.set_param(key, value)
    if flag is not None:
        ctx.proj_import(flag, dr)
        ctx.contact_detect(prev, prev)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device=pos.device)
    ctx.assemble(pos, prev, vel, ref, spd=False, grad=F)
    return F.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. per-step identity
@pytest.mark.parametrize("name", ["drape", "balancing", "bouncing", "sliding"])
def test_matches_differences_of_the_assembled_gradient(name):
    """-sum_free p . (F(theta + h) - F(theta - h)) / 2h for a seeded random p at the scene's state, every key; the sign is that of tsl_param_grad
    (force = -F).  h = theta / 2: every key enters F linearly at fixed positions and a fixed constraint set, so the quotient is exact up to
    rounding."""
    s = _task_scene(name)
    ctx = s._ensure_ctx()
    state = s._state()
    pos, prev = state[0], state[1]
    if s.elastics:
        # constraints detected at the start-of-step positions (what the step saw), friction slip = the motion of the step
        ctx.contact_detect(prev, prev)
        flag, dr = ctx.proj_export()[:2]
        nvf, nee = ctx.contact_counts()
        assert nvf > 0 and nee == 0
    else:
        flag = dr = None
    kv = _keys_and_values(s)
    rng = np.random.default_rng(17)
    p = torch.tensor(rng.normal(size=3 * s.tot_NV), device=pos.device)
    frozen = s.frozen.to_numpy().reshape(-1) != 0
    pn = p.cpu().numpy()
    fd, scale = {}, {}
    for k, v in kv.items():
        h = 0.5 * abs(v) if v != 0 else 1.0
        dF = (_grad_at(ctx, state, flag, dr, k, v + h) - _grad_at(ctx, state, flag, dr, k, v - h)) / (2 * h)
        ctx.set_param(k, v)
        dF[frozen] = 0.0
        fd[k] = -float(np.dot(pn, dF))
        scale[k] = float(np.abs(pn * dF).sum())
    if flag is not None:
        ctx.proj_import(flag, dr)
        ctx.contact_detect(prev, prev)
    got = ctx.param_grads(pos, state[3], list(kv), p=p)
    nonzero = 0
    for k in kv:
        if scale[k] == 0.0:
            assert got[k] == 0.0, (k, got[k])
            continue
        nonzero += 1
        assert abs(got[k] - fd[k]) <= 1e-8 * abs(fd[k]), (name, k, got[k], fd[k])
    assert nonzero >= 3 * len(s.cloths)
    if name in ("balancing", "bouncing"):
        assert scale["k_contact"] > 0
    if name == "balancing":
        assert scale["mu_cloth_elastic"] > 0
        assert sum(scale[f"elastic{i}.{m}"] > 0 for i in range(len(s.elastics)) for m in ("mu", "lam")) >= 4
    if name == "sliding":
        assert scale["mu_cloth_cloth"] > 0


# ------------------------------------------------------------------------------------------------ 2. agreement with the reference's calls
def test_agrees_with_param_grad_and_friction_grad_after_reverse_steps():
    """Scene_sliding, a real system-identification sweep: after every reverse step the sum over the cloths of cloth<i>.Kb is tsl_param_grad's kb
    and mu_cloth_cloth is tsl_friction_grad, both with p = the step's adjoint solution (p_dev = NULL)."""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    from thinshelllab_amd.engine.geometry import projection_query
    s = _task_scene("sliding")
    T = 2
    g = Grad(s, T, s.gripper.n_part); g.init_mass(s)
    g.copy_pos(s, 0)
    dpos = np.zeros((s.gripper.n_part, 3)); dpos[:, 0] = 2e-4
    for f in range(1, T):
        s.action(f, dpos, np.zeros_like(dpos))
        s.time_step(projection_query, f)
        g.copy_pos(s, f)
    g.get_loss_slide(s)
    ctx = s._ensure_ctx()
    kb_keys = [f"cloth{i}.Kb" for i in range(len(s.cloths))]
    seen = 0
    for st in range(T - 1, 0, -1):
        g.transfer_grad(st, s, projection_query)
        pos, ref = g.pos_buffer.t[st], g.ref_angle_buffer.t[st - 1]
        got = ctx.param_grads(pos, ref, kb_keys + ["mu_cloth_cloth"])
        kb = ctx.param_grad(pos, ref)["kb"]
        fr = ctx.friction_grad(pos)
        kb_sum = sum(got[k] for k in kb_keys)
        assert abs(kb_sum - kb) <= 1e-12 * abs(kb), (st, kb_sum, kb)
        assert abs(got["mu_cloth_cloth"] - fr) <= 1e-12 * abs(fr), (st, got["mu_cloth_cloth"], fr)
        print("reverse step", st, "kb", kb, kb_sum, "friction", fr, got["mu_cloth_cloth"])
        assert kb != 0 and abs(fr) > 1e-12


# ------------------------------------------------------------------------------------------------ 3. whole-rollout differences
def _bar_rollout(sc, T, params, vel0=None, ee=0, keys=(), seed=None, k_contact=1000.0):
    ctx = en.bar_context(sc, k_contact=k_contact)
    ctx.set_param("cg_tol", 1e-13)
    ctx.set_param("contact_ee", ee)
    for k, v in params.items():
        ctx.set_param(k, v)
    NV = len(sc["x"])
    pos = torch.tensor(sc["x"], device="cuda")
    prev = pos.clone()
    vel = torch.zeros_like(pos)
    if vel0 is not None:
        vel[:] = torch.tensor(vel0, device="cuda")
    ref = torch.zeros(3, dtype=torch.float64, device="cuda")
    xs = [pos.clone()]
    ncs, sets = [], []
    for _ in range(1, T):
        ctx.step(pos, prev, vel, ref)
        xs.append(pos.clone())
        ncs.append(ctx.contact_counts())
        sets.append(np.sort(ctx.constraints()["idx"], axis=0))
    L = float((seed * xs[-1]).sum().item())
    if not keys:
        ctx.close()
        return L, ncs, None
    pb = torch.stack(xs).contiguous()
    pg = torch.zeros_like(pb)
    pg[T - 1] = seed
    rb = torch.zeros((T, 3), dtype=torch.float64, device="cuda"); ag = torch.zeros_like(rb)
    tz = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
    ctx.set_param("adj_clamp", 1e30)
    tot = {k: 0.0 for k in keys}
    for s_ in range(T - 1, 0, -1):
        ctx.adjoint_step(s_, T, pb, pg, rb, ag, tz, 1.0)
        # the reverse step re-detects at x_{s-1}: the same constraints the forward step s used (the set this call differentiates against)
        assert np.array_equal(np.sort(ctx.constraints()["idx"], axis=0), sets[s_ - 1]), s_
        for k, v in ctx.param_grads(pb[s_], rb[s_ - 1], keys).items():
            tot[k] += v
    ctx.close()
    return L, ncs, tot


def _fd_check(sc, T, base, keys, tol, rel_h, **kw):
    NV = len(sc["x"])
    seed = torch.tensor(np.random.default_rng(4).normal(size=(NV, 3)), device="cuda")
    seed[: sc["n_lower"]] = 0.0
    _, ncs, g = _bar_rollout(sc, T, base, keys=keys, seed=seed, **kw)
    errs = {}
    for k in keys:
        h = rel_h * base[k]
        Lp, ncp, _ = _bar_rollout(sc, T, {**base, k: base[k] + h}, seed=seed, **kw)
        Lm, ncm, _ = _bar_rollout(sc, T, {**base, k: base[k] - h}, seed=seed, **kw)
        assert ncp == ncs and ncm == ncs, (k, ncs, ncp, ncm)
        fd = (Lp - Lm) / (2 * h)
        errs[k] = abs(g[k] - fd) / abs(fd)
        assert abs(fd) > 0 and errs[k] <= tol, (k, g[k], fd, errs[k])
    return ncs, errs


def test_rollout_differences_elastic_keys_contact_free():
    """upper bar (Neo-Hookean with log J) falling free for 4 steps: elastic0/1.mu and .lam against central differences of a random linear loss"""
    sc = en.bar_scene(gap=4e-3, mu_el=2e3, lam_el=3e3)
    base = {"elastic1.mu": 2e3, "elastic1.lam": 3e3}
    NV, nl = len(sc["x"]), sc["n_lower"]
    v0 = np.zeros((NV, 3)); v0[nl:] = np.random.default_rng(6).normal(scale=0.05, size=(NV - nl, 3))   # the bar deforms as it falls
    ncs, errs = _fd_check(sc, 4, base, list(base), 1e-4, 1e-3, vel0=v0)
    assert all(c == (0, 0) for c in ncs)
    print("elastic keys, contact-free rollout:", errs)


def _pressed_bars(mu):
    """parallel bars, the upper one shifted sideways so that its lower ridge rests on the lower bar's slanted face (vertex-triangle contact
    both ways), pressed in by 0.7 eps_contact"""
    sc = en.bar_scene(gap=0.0, angle=0.0, mu=mu)
    h = 0.01 / np.sqrt(2)
    nl = sc["n_lower"]
    sc["x"] = sc["x"].copy()
    sc["x"][nl:, 1] += 0.5 * h
    sc["x"][nl:, 2] += -0.5 * h + 0.7e-3 * np.sqrt(2)
    return sc


def test_rollout_differences_k_contact_frictionless():
    """mu = 1e-9 rather than 0 (the friction-lag adjoint of the reference divides c_k by mu).  h = 1e-3 k_contact: at 1e-4 the loss difference
    (5e-9 of a loss of order 0.1) is within the Newton tolerance of the steps (last |dx| / dt ~ 1e-8): 7e-2 apart there, 5e-5 at 1e-3,
    2e-3 at 1e-2 (the O(h^2) term).  The reverse steps re-detect the forward steps' constraints exactly (checked in _bar_rollout)."""
    sc = _pressed_bars(1e-9)
    ncs, errs = _fd_check(sc, 4, {"k_contact": 1000.0}, ["k_contact"], 1e-3, 1e-3, k_contact=1000.0)
    assert any(c[0] > 0 for c in ncs) and all(c[1] == 0 for c in ncs), ncs
    print("k_contact, frictionless rollout:", errs, ncs)


def test_rollout_differences_friction_keys_slip():
    """the pressed bars with live friction parameters (lower -> upper: mu_cloth_elastic, upper -> lower: mu_cloth_cloth), the upper bar sliding
    along at 0.1 m/s (slip well above eps_v): friction keys within 10 % (the lagged records c_k, dx0 are not differentiated)"""
    sc = _pressed_bars(0.5)
    NV, nl = len(sc["x"]), sc["n_lower"]
    sc["pairs"] = [(0, nl, NV, None, 1.0), (1, 0, nl, "cloth_cloth")]
    v0 = np.zeros((NV, 3)); v0[nl:, 0] = 0.1
    base = {"mu_cloth_elastic": 0.5, "mu_cloth_cloth": 0.3}
    ncs, errs = _fd_check(sc, 4, base, list(base), 0.1, 1e-3, vel0=v0)
    print("friction keys, slip rollout:", errs)


def test_rollout_differences_cloth_keys_drape():
    """cloth keys over whole drape rollouts.  The adjoint solves with the reference's Hessian, which has a factor-2 slip in the area block and
    slot-indexed bending terms (test_gpu_adjoint.py), so the whole-rollout derivative is not exact for cloth (measured: Kl 45 %,
    Ka 71 % apart): the signs, and Kb within the 15 % of the existing kb check.  What bounds the whole-rollout cloth derivative is the adjoint
    vector p of the reverse step, not this call: the per-step vector-Jacobian product itself is exact (test 1)."""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    T, N, sc_ = 4, 12, 1e-4
    base = dict(Kl=1000.0, Ka=1000.0, Kb=100.0)

    def rollout(vals, keys=()):
        s = Scene(cloth_size=0.1 / 15 * N, N=N, M=N, Kb=vals["Kb"], k_angle=3.14, perturb=2e-3, newton_cap=200)
        s.cloths[0].Kl[None] = vals["Kl"]; s.cloths[0].Ka[None] = vals["Ka"]
        s.init_all()
        s._ensure_ctx().set_param("cg_tol", 1e-13)
        g = Grad(s, T, 0); g.init_mass(s)
        g.param_keys = list(keys)
        g.copy_pos(s, 0)
        for f in range(1, T):
            s.time_step(None, f)
            g.copy_pos(s, f)
        c = s.cloths[0]
        z = g.pos_buffer.t[T - 1, c.offset:c.offset + c.NV, 2]
        L = float(sc_ * (z * z).sum().item() * 1e4 + sc_ * z.sum().item())
        if not keys:
            return L
        g.pos_grad.t[T - 1, c.offset:c.offset + c.NV, 2] = sc_ * (2e4 * z + 1.0)
        for st in range(T - 1, 0, -1):
            g.transfer_grad(st, s, None)
            assert g.pos_grad.t[st - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, dict(g.grad_params), g.grad_kb.value

    keys = ["cloth0.Kl", "cloth0.Ka", "cloth0.Kb"]
    _, gp, kb = rollout(base, keys)
    assert gp["cloth0.Kb"] == kb or abs(gp["cloth0.Kb"] - kb) <= 1e-12 * abs(kb)
    errs, fds = {}, {}
    for k in keys:
        f = k.split(".")[1]
        h = 0.02 * base[f]
        fds[k] = (rollout({**base, f: base[f] + h}) - rollout({**base, f: base[f] - h})) / (2 * h)
        errs[k] = abs(gp[k] - fds[k]) / abs(fds[k])
    print("cloth keys, drape rollout:", errs)
    assert all(gp[k] * fds[k] > 0 for k in keys), (gp, fds)
    assert errs["cloth0.Kb"] <= 0.15, errs


# ------------------------------------------------------------------------------------------------ 4. invariance and determinism
def _sweep(keys_per_step, patch=None):
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    from thinshelllab_amd.engine.geometry import projection_query
    s = _task_scene("balancing")
    T = 3
    g = Grad(s, T, s.gripper.n_part); g.init_mass(s)
    g.count_mu_lam_grad = True
    g.param_keys = keys_per_step
    g.copy_pos(s, 0)
    for f in range(1, T):
        s.time_step(projection_query, f)
        g.copy_pos(s, f)
    g.get_loss_slide(s)
    for st in range(T - 1, 0, -1):
        g.transfer_grad(st, s, projection_query)
    return g


def test_one_key_equals_all_keys_shuffled_and_runs_repeat():
    s = _task_scene("balancing")
    ctx = s._ensure_ctx()
    pos, prev, vel, ref = s._state()
    p = torch.tensor(np.random.default_rng(9).normal(size=3 * s.tot_NV), device=pos.device)
    keys = list(_keys_and_values(s))
    shuffled = keys[:]
    random.Random(5).shuffle(shuffled)
    all1 = ctx.param_grads(pos, ref, shuffled, p=p)
    all2 = ctx.param_grads(pos, ref, keys, p=p)
    for k in keys:
        one = ctx.param_grads(pos, ref, [k], p=p)[k]
        assert one == all1[k] == all2[k], k
    g1 = _sweep(keys)
    g2 = _sweep(shuffled)
    assert g1.grad_params == g2.grad_params and any(v != 0 for v in g1.grad_params.values())


def test_empty_keys_never_call_the_new_function(monkeypatch):
    from thinshelllab_amd.context import TslContext
    g0 = _sweep([])

    def boom(*a, **k):
        raise AssertionError("param_grads called with param_keys empty")

    monkeypatch.setattr(TslContext, "param_grads", boom)
    g1 = _sweep([])
    assert g1.grad_params == {} and g0.grad_params == {}
    assert torch.equal(g0.pos_grad.t, g1.pos_grad.t) and torch.equal(g0.pos_buffer.t, g1.pos_buffer.t)
    assert g0.grad_kb.value == g1.grad_kb.value and g0.grad_mu.value == g1.grad_mu.value and g0.grad_lam.value == g1.grad_lam.value
    g0.reset()
    assert g0.grad_params == {}


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors_name_the_key():
    from thinshelllab_amd._lib import TslError
    s = _task_scene("drape")
    ctx = s._ensure_ctx()
    pos, _, _, ref = s._state()
    for k in ("no_such_key", "eps_contact", "damping", "cloth0.k_angle", "elastic0.mu", "cloth1.Kl", "cloth-1.Kb", "cg_tol", "cloth+0.Kl", "cloth 0.Kl"):
        with pytest.raises(TslError, match=re.escape(k)):
            ctx.param_grads(pos, ref, ["cloth0.Kl", k])
    assert ctx.param_grads(pos, ref, []) == {}
    # tsl_set_param reads the same keys through the same parser: a malformed or out-of-range index and an unknown field fail, naming the key
    for k in ("cloth+0.Kl", "cloth 0.Kl", "cloth1.Kl", "cloth0.nope"):
        with pytest.raises(TslError, match=re.escape(k)):
            ctx.set_param(k, 1.0)


def test_edge_edge_slots_fail_the_keys_they_would_need():
    """crossing bars with edge-edge constraints of the mu_cloth_cloth pairs: k_contact and mu_cloth_cloth fail, mu_cloth_elastic (no slot of
    its kind) and the material keys work"""
    sc = en.bar_scene(gap=2e-4)
    NV, nl = len(sc["x"]), sc["n_lower"]
    sc["pairs"] = [(0, nl, NV, "cloth_cloth"), (1, 0, nl, "cloth_cloth")]
    ctx = en.bar_context(sc)
    ctx.set_param("contact_ee", 1)
    pos = torch.tensor(sc["x"], device="cuda")
    ctx.contact_detect(pos, pos.clone())
    assert ctx.contact_counts()[1] > 0
    ref = torch.zeros(3, dtype=torch.float64, device="cuda")
    p = torch.ones(3 * NV, dtype=torch.float64, device="cuda")
    from thinshelllab_amd._lib import TslError
    for k in ("k_contact", "mu_cloth_cloth"):
        with pytest.raises(TslError, match=k):
            ctx.param_grads(pos, ref, [k], p=p)
    assert ctx.param_grads(pos, ref, ["mu_cloth_elastic", "elastic1.mu"], p=p)["mu_cloth_elastic"] == 0.0
    ctx.set_param("contact_ee", 0)
    ctx.contact_detect(pos, pos.clone())
    ctx.param_grads(pos, ref, ["k_contact", "mu_cloth_cloth"], p=p)
    ctx.close()
