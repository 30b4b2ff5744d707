"""Rigid frames for soft handles (tsl_set_handle_frames, tsl_set_frame_poses, tsl_frame_wrench, tsl_frame_grad; csrc/k_frame.hpp).
Frames rewrite rows of the target buffer the handle kernels read and reduce per-handle rows to six numbers per frame.  Checked against the NumPy
restatement (tests/frame_numpy.py) applied to the outputs of the handle read-outs, against a context whose targets were set by hand (bit for bit:
nothing but the targets may differ), and against central differences of whole rollouts in the pose of every step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_numpy as fn  # noqa: E402

pytestmark = pytest.mark.gpu

K = 2.0e5    # N/m, the per-state checks (the stiffness of tests/test_gpu_handles.py)
KD = 2000.0  # N/m, steps and rollouts
T_TAPE = 6
POSE_SCALE_FD = 0.3   # the whole-rollout differences: the frame's steps of the T = 6 drape scaled to those of the handle rollout test (0.3 to 0.6 mm at the corners)
SIZES = [64, 1, 0, 257, 65]   # handles per frame: a full wave, a single lane, none, one pass past the 256-lane stride, one lane into the second wave
N_FREE = 10


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


def _lists(rng):
    """397 handles on the 441 vertices of an N = 20 cloth in shuffled order: frames of SIZES handles and N_FREE free ones, weights with zeros"""
    n = sum(SIZES) + N_FREE
    v = rng.permutation(441)[:n].astype(np.int32)
    frame_of = np.concatenate([np.full(m, j) for j, m in enumerate(SIZES)] + [np.full(N_FREE, -1)]).astype(np.int32)
    frame_of = frame_of[rng.permutation(n)]
    w = rng.uniform(0.25, 2.0, n)
    w[rng.choice(n, 12, replace=False)] = 0.0
    w[frame_of == 1] = 1.3                                # (the single handle of frame 1 carries weight)
    return v, w, frame_of


def _unit_ball(rng, n, radius):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None] * radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)


@pytest.fixture(scope="module")
def fx():
    """the context of the per-state checks: handles, random local points |r| <= 0.1, random poses |c| <= 1 with rotations of any angle"""
    rng = np.random.default_rng(20)
    s = _cloth(20)
    assert s.tot_NV == 441
    v, w, frame_of = _lists(rng)
    local = _unit_ball(rng, len(v), 0.1)
    local[frame_of == -1] = np.nan                      # (the point of a free handle is never read)
    pos = _unit_ball(rng, len(SIZES), 1.0)
    quat = rng.normal(size=(len(SIZES), 4)) * rng.uniform(0.5, 3.0, (len(SIZES), 1))   # not normalised: the library does that
    t_world = rng.normal(scale=0.5, size=(len(v), 3))
    x = s.pos.to_numpy() + rng.normal(scale=0.15 * s.cloths[0].dx, size=(441, 3))
    ctx = s._ensure_ctx()
    ctx.set_handles(v, w)
    ctx.set_param("k_handle", K)
    yield dict(s=s, ctx=ctx, v=v, w=w, frame_of=frame_of, local=local, pos=pos, quat=quat, t_world=t_world, x=x, rng=rng)
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ 1. targets
def test_targets_match_the_restatement_whatever_the_order_of_the_calls(fx):
    ctx, fo = fx["ctx"], fx["frame_of"]
    free = fo == -1
    ctx.set_handle_targets(fx["t_world"])
    ctx.set_handle_frames(fo, fx["local"], len(SIZES))
    t0 = ctx.handle_targets()
    assert np.array_equal(t0[~free], fx["local"][~free])        # poses start at the identity at the origin: t = 0 + 1 r
    assert np.array_equal(t0[free], fx["t_world"][free])
    ctx.set_frame_poses(fx["pos"], fx["quat"])
    t1 = ctx.handle_targets()
    want = fn.targets(fx["t_world"], fo, np.nan_to_num(fx["local"]), fx["pos"], fx["quat"])
    err = np.abs(t1 - want).max()
    print("targets: max |t - restatement| = %.3e m (bound 1e-14)" % err)
    assert err <= 1e-14
    assert np.array_equal(t1[free], fx["t_world"][free])        # rows of free handles: the bits that were set
    assert np.abs(t1[~free] - t0[~free]).max() > 0.1            # (the poses are no identities)
    ctx.set_handle_targets(fx["t_world"])                       # targets last: the framed rows follow their frames again
    assert np.array_equal(ctx.handle_targets(), t1)
    ctx.set_handle_targets(fx["t_world"] + 1.0)
    ctx.set_frame_poses(fx["pos"], fx["quat"])                  # poses last
    t2 = ctx.handle_targets()
    assert np.array_equal(t2[~free], t1[~free]) and np.array_equal(t2[free], fx["t_world"][free] + 1.0)
    ctx.set_handle_targets(fx["t_world"])


# ------------------------------------------------------------------------------------------------ 2. read-outs
def test_wrench_and_pose_gradient_match_the_restatement_of_the_handle_rows(fx):
    ctx, fo, v, rng = fx["ctx"], fx["frame_of"], fx["v"], np.random.default_rng(21)
    nf = len(SIZES)
    ctx.set_handle_targets(fx["t_world"])
    ctx.set_handle_frames(fo, fx["local"], nf)
    ctx.set_frame_poses(fx["pos"], fx["quat"])
    # frozen dofs: every handled dof of frame 0 (64 handles), single dofs in the other frames
    fz = np.zeros((441, 3), np.int32)
    fz[v[fo == 0]] = 1
    some = v[(fo == 3) | (fo == 4)]
    fz[some[::5], rng.integers(0, 3, len(some[::5]))] = 1
    ctx.set_frozen(fz.reshape(-1))
    pos = _dev(fx["x"])
    pn = rng.normal(size=3 * 441)
    p = _dev(pn)
    t = ctx.handle_targets()
    local = np.nan_to_num(fx["local"])
    for name, got, (want, mag) in (
            ("wrench", ctx.frame_wrench(pos), fn.wrench(ctx.handle_force(pos), t, fo, fx["pos"])),
            ("grad", ctx.frame_grad(p), fn.pose_grad(ctx.handle_grad(p), fo, local, fx["quat"], nf))):
        rel = np.abs(got - want) / np.where(mag > 0, mag, 1.0)
        print("frame_%s: max |got - restatement| / sum |terms| = %.3e (bound 1e-12); largest entry %.3e" % (name, rel.max(), np.abs(got).max()))
        assert (np.abs(got - want) <= 1e-12 * mag).all()
        assert got.shape == (nf, 6) and (got[2] == 0).all()     # the frame without handles: exact zeros
    wr, fg = ctx.frame_wrench(pos), ctx.frame_grad(p)
    assert (fg[0] == 0).all() and (wr[0] != 0).all()            # all handled dofs frozen: no gradient; the wrench is not masked
    assert (fg[[1, 3, 4]] != 0).all()
    assert np.array_equal(wr, ctx.frame_wrench(pos)) and np.array_equal(fg, ctx.frame_grad(p))   # the same bits call after call
    # the handle read-outs are what they were without frames: the rows of a context whose targets were set by hand
    f_rows, g_rows = ctx.handle_force(pos), ctx.handle_grad(p)
    ctx.set_handle_frames(None, None, 0)
    ctx.set_handle_targets(t)
    assert np.array_equal(ctx.handle_targets(), t)
    assert np.array_equal(ctx.handle_force(pos), f_rows) and np.array_equal(ctx.handle_grad(p), g_rows)
    assert ctx.frame_wrench(pos).shape == (0, 6) and ctx.frame_grad(p).shape == (0, 6)
    # k_handle = 0: zeros
    ctx.set_handle_frames(fo, fx["local"], nf)
    ctx.set_frame_poses(fx["pos"], fx["quat"])
    ctx.set_param("k_handle", 0.0)
    assert (ctx.frame_wrench(pos) == 0).all() and (ctx.frame_grad(p) == 0).all() and ctx.frame_wrench(pos).shape == (nf, 6)
    ctx.set_param("k_handle", K)
    assert np.array_equal(ctx.frame_wrench(pos), wr)
    ctx.set_frozen(np.zeros(3 * 441, np.int32))


# ------------------------------------------------------------------------------------------------ 3. nothing else moved
def _everything(s, x, wgt, p):
    """energy, gradient, matrix, the k_handle key at a state, then one step and one reverse step from the scene's own state"""
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    ctx = s._ensure_ctx()
    pos = _dev(x); prev = pos.clone(); vel = torch.zeros_like(pos)
    F = torch.zeros(pos.numel(), dtype=torch.float64, device="cuda")
    ctx.assemble(pos, prev, vel, s._ref_angle, spd=1, grad=F)
    out = [F.cpu().numpy(), ctx.matrix()[2].copy(), np.float64(ctx.energy(pos, prev, vel, s._ref_angle)),
           np.float64(ctx.param_grads(pos, s._ref_angle, ["k_handle"], p=p)["k_handle"])]
    g = Grad(s, 2, 0); g.init_mass(s)
    g.copy_pos(s, 0)
    st = s.time_step(None, 1)
    assert st["unconverged"] == 0 and st["newton_iters"] < 200, st
    g.copy_pos(s, 1)
    g.pos_grad.t[1] = _dev(wgt)
    g.transfer_grad(1, s, None)
    assert g.last_stats["flag"] != 3
    out += [g.pos_buffer.t.cpu().numpy().copy(), s.vel.to_numpy(), g.pos_grad.t.cpu().numpy().copy(), g.handle_grad.t.numpy().copy(),
            np.float64(st["newton_iters"])]
    return out, g


def test_a_context_on_frames_equals_one_whose_targets_were_set_by_hand():
    rng = np.random.default_rng(22)
    v, w, fo = _lists(rng)
    nf = len(SIZES)
    wgt = rng.normal(scale=1e-2, size=(441, 3))
    p = _dev(rng.normal(size=3 * 441))
    # the frames grasp the vertices where they are, then move a little: a pull a step can follow
    cpos = _unit_ball(rng, nf, 0.05) + [0.07, 0.07, 0.0]
    dth = rng.normal(scale=0.01, size=(nf, 3))
    A = _cloth(20); B = _cloth(20)
    x0 = A.pos.to_numpy()
    x = x0 + rng.normal(scale=1e-4, size=x0.shape)
    t_free = x0[v] + rng.normal(scale=1e-3, size=(len(v), 3))
    for s in (A, B):
        s._ensure_ctx().set_param("direct", 1)
        s.set_handles(v, KD, w)
        s.set_handle_targets(t_free)
    A.set_handle_frames(fo, n_frames=nf)
    A.set_frame_poses(cpos, np.tile([1.0, 0.0, 0.0, 0.0], (nf, 1)))
    A.set_handle_frames(fo)                                      # r_i = x_i - c
    A.move_frames(rng.normal(scale=1e-3, size=(nf, 3)), dth)
    assert A.n_frame == nf
    t = A._ensure_ctx().handle_targets()
    assert np.abs(t - A._handle_t).max() <= 1e-15 and 1e-4 < np.abs(t - x0[v]).max() < 1e-2
    B.set_handle_targets(t)
    a, ga = _everything(A, x, wgt, p)
    b, gb = _everything(B, x, wgt, p)
    for i, (ai, bi) in enumerate(zip(a, b)):
        assert np.array_equal(ai, bi), i
    assert np.abs(a[7]).max() > 0 and np.abs(ga.frame_grad.t[1].numpy()[[0, 1, 3, 4]]).min() > 0 and not hasattr(gb, "frame_grad")
    wr = A.frame_wrench()
    assert wr.shape == (nf, 6) and (wr[2] == 0).all() and np.abs(wr[[0, 3, 4]]).min() > 0
    # frames removed: the context is one that never had any (B never had; same state, same new targets)
    t2 = x0[v] + rng.normal(scale=1e-3, size=(len(v), 3))
    A.set_handle_frames([], n_frames=0)
    ctxA = A._ensure_ctx()
    assert A.n_frame == 0 and ctxA.n_frame == 0
    for s in (A, B):
        s.pos.from_numpy(x0); s.prev_pos.from_numpy(x0); s.vel.fill(0.0)
        s.set_handle_targets(t2)
    assert np.array_equal(A._ensure_ctx().handle_targets(), t2)
    a, _ = _everything(A, x, wgt, p)
    b, _ = _everything(B, x, wgt, p)
    for i, (ai, bi) in enumerate(zip(a, b)):
        assert np.array_equal(ai, bi), i
    # tsl_set_handles drops the frames
    ctxB = B._ensure_ctx()
    ctxB.set_handle_frames(fo, np.zeros((len(v), 3)), nf)
    assert ctxB.n_frame == nf and not np.array_equal(ctxB.handle_targets(), t)
    ctxB.set_handles(v, w)
    ctxB.set_handle_targets(t2)
    assert ctxB.n_frame == 0 and np.array_equal(ctxB.handle_targets(), t2)
    ctxB.set_frame_poses(np.zeros((0, 3)), np.zeros((0, 4)))
    assert np.array_equal(ctxB.handle_targets(), t2)
    for s in (A, B):
        s._close_ctx()


# ------------------------------------------------------------------------------------------------ 4. errors
def test_errors_name_the_offender():
    from thinshelllab_amd._lib import TslError
    s = _cloth(12)
    ctx = s._ensure_ctx()
    with pytest.raises(TslError, match=r"2 frames asked for, but there are no handles"):
        ctx.set_handle_frames(np.zeros(0, np.int32), np.zeros((0, 3)), 2)
    ctx.set_handles([3, 5, 8, 13])
    ok_f, ok_r = np.array([0, -1, 1, 1], np.int32), np.array([[0.0, 0, 0], [np.inf, 0, 0], [0, 0.1, 0], [0, 0, 0.1]])
    with pytest.raises(TslError, match=r"frame index 2 of handle 3 outside \[-1, 2\)"):
        ctx.set_handle_frames([0, -1, 1, 2], ok_r, 2)
    with pytest.raises(TslError, match=r"frame index -2 of handle 0 outside \[-1, 2\)"):
        ctx.set_handle_frames([-2, -1, 1, 1], ok_r, 2)
    bad_r = ok_r.copy(); bad_r[2, 2] = np.nan
    with pytest.raises(TslError, match=r"local point \(0, 0\.1, nan\) of handle 2 \(frame 1\) is not finite"):
        ctx.set_handle_frames(ok_f, bad_r, 2)
    ctx.set_handle_frames(ok_f, ok_r, 2)          # valid: the non-finite point belongs to a free handle
    with pytest.raises(TslError, match=r"quaternion \(0, 0, 0, 0\) of frame 1 is zero or not finite"):
        ctx.set_frame_poses(np.zeros((2, 3)), [[1.0, 0, 0, 0], [0.0, 0, 0, 0]])
    with pytest.raises(TslError, match=r"quaternion \(1, 0, inf, 0\) of frame 0 is zero or not finite"):
        ctx.set_frame_poses(np.zeros((2, 3)), [[1.0, 0, np.inf, 0], [1.0, 0, 0, 0]])
    # a refused call leaves the frames and the poses as they were
    t = ctx.handle_targets()
    assert np.array_equal(t[[0, 2, 3]], ok_r[[0, 2, 3]]) and ctx.n_frame == 2
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ 5. / 6. the drape held by a frame
# The sheet of the handle rollouts (tests/test_gpu_handles.py): 16 x 16, StVK membrane, Kb = 0, flat from rest, the two corners of grid row N on
# handles -- here both on one frame that sits off the line through them, so that every axis of rotation moves them.
def _drape(direct=1, cg_tol=None, frames=True):
    s = _cloth(16, pin=False, perturb=0.0, Kb=0.0, stvk=(3.0e5, 2.0e5))
    held = s.cloths[0].corner_ids()[2:]
    s.set_handles(held, KD)
    if frames:
        s.set_handle_frames([0, 0], n_frames=1)
        s.set_frame_poses(s.pos.to_numpy()[held].mean(0)[None] + [0.0, 0.0, 0.02], [[1.0, 0.0, 0.0, 0.0]])
        s.set_handle_frames([0, 0])
    ctx = s._ensure_ctx()
    ctx.set_param("direct", direct)
    if cg_tol:
        ctx.set_param("cg_tol", cg_tol)
    return s


def _poses(s, T, scale=1.0):
    """(T, 1, 3) positions and (T, 1, 4) quaternions: per step the frame moves up and out and turns about a skew axis (1 to 2 mm at the corners)"""
    from thinshelllab_amd.engine.frames import compose
    pos, quat = s.frame_poses()
    P, Q = [pos], [quat]
    for _ in range(1, T):
        pos, quat = compose(pos, quat, scale * np.array([[1e-4, -1e-4, 3e-4]]), scale * np.array([[0.01, -0.02, 0.015]]))
        P.append(pos); Q.append(quat)
    return np.array(P), np.array(Q)


def _reset(s, x0):
    s.pos.from_numpy(x0); s.prev_pos.from_numpy(x0); s.vel.fill(0.0)


def _forward(s, g, T, poses=None, targets=None, read=None):
    def put(f):
        if poses is not None:
            s.set_frame_poses(poses[0][f], poses[1][f])
        if targets is not None:
            s.set_handle_targets(targets[f])
        if read is not None:
            read.append(s._ensure_ctx().handle_targets())
    put(0)
    g.copy_pos(s, 0)
    for f in range(1, T):
        put(f)
        st = s.time_step(None, f)
        assert st["unconverged"] == 0 and st["newton_iters"] < 200, st
        g.copy_pos(s, f)


def _reverse(s, g, wgt, T):
    g.pos_grad.t[T - 1] = _dev(wgt)
    for f in range(T - 1, 0, -1):
        g.transfer_grad(f, s, None)
        assert g.last_stats["flag"] != 3


def test_drape_on_a_frame_repeats_equals_hand_set_targets_and_group_members_equal_single_runs():
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.scene_group import SceneGroup
    T = T_TAPE
    wgt = np.random.default_rng(7).normal(scale=1e-2, size=(289, 3))
    runs, read = [], []
    for scale in (1.0, 1.0, 0.5):
        s = _drape()
        g = Grad(s, T, 0); g.init_mass(s)
        read = []
        _forward(s, g, T, poses=_poses(s, T, scale), read=read if scale == 1.0 else None)
        _reverse(s, g, wgt, T)
        runs.append((g.pos_buffer.t.cpu().numpy().copy(), g.frame_grad.t.numpy().copy(), g.handle_grad.t.numpy().copy(), np.array(read)))
        s._close_ctx()
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert np.abs(runs[0][0][-1] - runs[0][0][0]).max() > 1e-4 and np.abs(runs[0][1][1:]).min() > 0 and not np.array_equal(runs[0][0], runs[2][0])
    assert (runs[0][1][0] == 0).all()
    # the same world targets set by hand, no frames: the same tape and the same handle rows
    s = _drape(frames=False)
    g = Grad(s, T, 0); g.init_mass(s)
    _forward(s, g, T, targets=runs[0][3])
    _reverse(s, g, wgt, T)
    assert np.array_equal(g.pos_buffer.t.cpu().numpy(), runs[0][0]) and np.array_equal(g.handle_grad.t.numpy(), runs[0][2]) and g.n_frame == 0
    s._close_ctx()
    # S = 2, the members on different poses
    ms = [_drape(), _drape()]
    ps = [_poses(ms[0], T, 1.0), _poses(ms[1], T, 0.5)]
    G = SceneGroup(ms)
    gs = []
    for m, pq in zip(ms, ps):
        g = Grad(m, T, 0); g.init_mass(m)
        m.set_frame_poses(pq[0][0], pq[1][0]); g.copy_pos(m, 0)
        gs.append(g)
    for f in range(1, T):
        for m, pq in zip(ms, ps):
            m.set_frame_poses(pq[0][f], pq[1][f])
        sts = G.time_step(None, f)
        assert all(r["unconverged"] == 0 for r in sts)
        for m, g in zip(ms, gs):
            g.copy_pos(m, f)
    for g in gs:
        g.pos_grad.t[T - 1] = _dev(wgt)
    for f in range(T - 1, 0, -1):
        G.transfer_grad(f, gs, None)
    G.close()
    for i, j in ((0, 0), (1, 2)):
        assert np.array_equal(gs[i].pos_buffer.t.cpu().numpy(), runs[j][0]), i
        assert np.array_equal(gs[i].frame_grad.t.numpy(), runs[j][1]), i
        assert np.array_equal(gs[i].handle_grad.t.numpy(), runs[j][2]), i
        assert np.array_equal(gs[i].frame_pos.t.numpy(), ps[i][0]) and np.array_equal(gs[i].frame_quat.t.numpy(), ps[i][1]), i
    for m in ms:
        m._close_ctx()


def test_whole_rollout_pose_gradients_match_differences():
    """T = 4 on the frame-held drape, analytic_grad_system.Grad (clamp at 1, inactive: the loss weights are 1e-2), a random linear loss on the last
    state.  frame_grad[s] for every step against central differences of the loss over whole rollouts in c_s and in a world rotation vector applied
    on the left of R_s, at two step sizes a decade apart.  Bound per block: the larger of 1e-3 of the block's largest entry (the cap of the handle
    rollout test: frame_grad is a fixed linear map of handle_grad, measured there at 4.6e-4) and three times the disagreement of the two
    differences.  Measured when this test was written: see the figures in DESIGN.md 2.5."""
    from thinshelllab_amd.engine.analytic_grad_system import Grad
    from thinshelllab_amd.engine.frames import compose
    T = 4
    s = _drape(cg_tol=1e-13)
    x0 = s.pos.to_numpy()
    P0, Q0 = _poses(s, T, POSE_SCALE_FD)
    wgt = np.random.default_rng(8).normal(scale=1e-2, size=x0.shape)

    def rollout(P, Q, reverse=False, late=False):
        _reset(s, x0)
        g = Grad(s, T, 0); g.init_mass(s)
        _forward(s, g, T, poses=(P, Q))
        L = float((g.pos_buffer.t[T - 1].cpu().numpy() * wgt).sum())
        if not reverse:
            return L
        if late:   # the poses reach the reverse sweep one step late
            g.frame_pos.t[1:] = torch.as_tensor(P[:-1]); g.frame_quat.t[1:] = torch.as_tensor(Q[:-1])
        g.pos_grad.t[T - 1] = _dev(wgt)
        for f in range(T - 1, 0, -1):
            g.transfer_grad(f, s, None)
            assert g.pos_grad.t[f - 1].abs().max().item() < 1.0, "clamp would be active"
        return L, g.frame_grad.t.numpy().copy()

    _, fg = rollout(P0, Q0, reverse=True)

    def cd(f, a, h):
        out = []
        for sign in (1.0, -1.0):
            P, Q = P0.copy(), Q0.copy()
            d = np.zeros((1, 6)); d[0, a] = sign * h
            P[f], Q[f] = compose(P0[f], Q0[f], d[:, :3], d[:, 3:])
            out.append(rollout(P, Q))
        return (out[0] - out[1]) / (2 * h)

    fd = np.zeros((2,) + fg.shape)
    # metres for c, radians for theta (arms of 6 cm: the same displacements).  Small steps: the sheet has no bending stiffness, and the truncation
    # error of a central difference was 15 % of the position block at h = 3e-5 m and 0.2 % at 3e-6 m when this test was written
    for n, (hc, hr) in enumerate(((3e-6, 5e-5), (3e-7, 5e-6))):
        for f in range(1, T):
            for a in range(6):
                fd[n, f, 0, a] = cd(f, a, hc if a < 3 else hr)
    ok = True
    err_late = {}
    _, fg_late = rollout(P0, Q0, reverse=True, late=True)
    for name, sl in (("position", slice(0, 3)), ("rotation", slice(3, 6))):
        big = np.abs(fd[1][..., sl]).max()
        disagree = np.abs(fd[0][..., sl] - fd[1][..., sl]).max()
        err = np.abs(fg[..., sl] - fd[1][..., sl]).max()
        bound = max(1e-3 * big, 3 * disagree)
        err_late[name] = (np.abs(fg_late[..., sl] - fd[1][..., sl]).max(), bound)
        print("frame_grad %s block: max |entry| %.4e, the two differences disagree by %.2e (%.2e relative), analytic - difference %.2e (%.2e relative), "
              "bound %.2e; poses one step late: %.2e (%.2e relative)" % (name, big, disagree, disagree / big, err, err / big, bound, err_late[name][0], err_late[name][0] / big))
        ok = ok and err <= bound
    assert (fg[0] == 0).all()
    assert ok
    assert err_late["rotation"][0] > err_late["rotation"][1]    # the reverse step reads the poses of its own step
    s._close_ctx()


# ------------------------------------------------------------------------------------------------ 7. driver
def test_trajopt_driver_lowers_the_loss():
    from thinshelllab_amd.training.trajopt_frames import optimise
    losses, steps = optimise(N=8, T=4, iters=3, log=print)
    assert len(losses) == 3 and losses[1] < losses[0] and losses[2] < losses[1], losses
    assert steps.shape == (4, 1, 6) and np.abs(steps[1:]).max() > 0 and (steps[0] == 0).all()
