"""The context key "spd_literal" (include/tsl_hip.h): with it set, the forward projections of the cloth spring blocks (3 x 3, K = 10), the contact
normal blocks and the tactile element blocks (9 x 9, K = 20) run the reference's own projector -- SPD_Projector, engine/linalg.py:15-148:
Householder tridiagonalisation, at most K shifted-QR sweeps, rebuild from the positive diagonal -- on the GPU (spd_literal3 / spd_literal9_coop,
csrc/tsl_device.hpp) instead of the converged eigen-clamp.  Checked against the oracle's restatement of the same arithmetic (oracle/tslo_linalg.h,
spd mode 0): block by block for the same bits, on the assembled operator of the native scenes, on the full-size fixture rollouts
(tests/golden/oracle_cfg{3,4}.npz were generated in the oracle's literal mode), and for determinism on the direct path and in scene groups."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=0.1 / 15 * 8, N=8, M=8)
    s.init_all()
    return s._ensure_ctx()


def _blocks(oracle, D, K, scale, seed):
    """random symmetric blocks, the special blocks of test_gpu_spd_project.py, blocks with a perturbed upper triangle, and (9 x 9) blocks on which the
    reference's projector stops at its sweep limit"""
    rng = np.random.default_rng(seed)
    n = 2000
    A = rng.normal(size=(n, D, D)) * scale
    A = 0.5 * (A + A.transpose(0, 2, 1))
    A[0] = np.eye(D) * scale
    A[1] = -np.eye(D) * scale
    A[2] = 0.0
    x = rng.normal(size=D); A[3] = np.outer(x, x) * scale - 0.3 * scale * np.eye(D)
    iu = np.triu_indices(D, 1)
    for i in range(4, n, 4):   # not symmetric: only the lower triangle may be read
        A[i][iu] += 1e-3 * scale * rng.normal(size=len(iu[0]))
    if D == 9 and scale >= 1e6:
        capped = []
        while len(capped) < 150:
            B = rng.normal(size=(2000, D, D)) * scale
            B = 0.5 * (B + B.transpose(0, 2, 1))
            capped += [b for b in B if oracle.spd_project(b, K)[1] == K]
        A = np.concatenate([A, np.array(capped)])
    return A


def _project(ctx, A, D):
    dev = torch.as_tensor(A, device="cuda").contiguous()
    ctx.spd_project(dev, D)
    return dev.cpu().numpy()


@pytest.mark.parametrize("D,K", [(3, 10), (9, 20)])
@pytest.mark.parametrize("scale", [1.0, 1e3, 1e6])
def test_literal_blocks_bit_identical_to_oracle(oracle, ctx, D, K, scale):
    oracle.set_spd_mode(0)
    A = _blocks(oracle, D, K, scale, 100 * D + int(np.log10(scale)))
    ref = np.empty_like(A)
    sweeps = np.empty(len(A), dtype=int)
    for i in range(len(A)):
        ref[i], sweeps[i] = oracle.spd_project(A[i], K)
    default = _project(ctx, A, D)
    try:
        ctx.set_param("spd_literal", 1)
        lit = _project(ctx, A, D)
    finally:
        ctx.set_param("spd_literal", 0)
    again = _project(ctx, A, D)
    scl = np.maximum(np.abs(A).reshape(len(A), -1).max(axis=1), 1e-300)
    dl = np.abs(lit - ref).reshape(len(A), -1).max(axis=1) / scl
    dd = np.abs(default - ref).reshape(len(A), -1).max(axis=1) / scl
    n_diff = int((lit != ref).reshape(len(A), -1).any(axis=1).sum())
    n_cap = int((sweeps == K).sum())
    print(f"\nD={D} scale={scale:g}: {len(A)} blocks ({n_cap} capped at K={K}); literal vs oracle: {n_diff} not bit-identical, max rel {dl.max():.2e}; "
          f"default (eigen-clamp) vs oracle: max rel {dd.max():.2e}")
    if D == 9 and scale >= 1e6:
        assert n_cap >= 100
    assert n_diff == 0, (n_diff, float(dl.max()), int(np.argmax(dl)))
    assert dd.max() > 1e-9, "the key did not switch the projector"
    assert np.array_equal(again, default), "the key set back to 0 does not give the default path"


def test_literal_key_accepts_0_and_1_only(ctx):
    from thinshelllab_amd._lib import TslError
    with pytest.raises(TslError):
        ctx.set_param("spd_literal", 2)
    ctx.set_param("spd_literal", 0)


def _operator_diff(oracle, s, o, spd):
    o.newton_step_init(); o.compute_energy(); o.compute_residual_and_Hessian(spd)
    s.compute_residual_and_Hessian(spd=spd)
    Hg = s._ctx.operator_csr().toarray(); Ho = o.H_csr().toarray()
    return np.abs(Hg - Ho).max(), np.abs(Ho).max()


@pytest.mark.parametrize("name", ["folding", "lifting", "balancing"])
def test_literal_operator_at_equal_states(oracle, name):
    """the assembled operator of the three native scenes with contact, spd on, oracle in its literal mode: the GPU's literal operator against the
    oracle's, next to the spd-off difference (the assembly's own rounding floor) and the default mode's (the eigen-clamp against the literal projector)"""
    import test_gpu_scenes as tgs
    from thinshelllab_amd.engine.geometry import projection_query
    s, o = tgs._pair(oracle, name)
    oracle.set_spd_mode(0)
    rng = np.random.default_rng(2)
    x = s.pos.to_numpy()
    xp = x + rng.normal(0, 2e-5, x.shape)
    fr = s.frozen.to_numpy().reshape(-1, 3).astype(bool)
    xp[fr] = x[fr]
    projection_query(s)
    o.calc_vn(); o.projection_query(); o.contact_analysis()
    assert o.nc > 0
    s.pos.from_numpy(xp); o.pos[:] = xp; o.push_down_all()
    floor, _ = _operator_diff(oracle, s, o, False)
    d_def, hmax = _operator_diff(oracle, s, o, True)
    s.set_spd_literal(True)
    d_lit, _ = _operator_diff(oracle, s, o, True)
    s.set_spd_literal(False)
    d_back, _ = _operator_diff(oracle, s, o, True)
    print(f"\n{name}: max |H_gpu - H_oracle| / |H|: spd off {floor / hmax:.3e}, literal {d_lit / hmax:.3e}, default (eigen-clamp) {d_def / hmax:.3e}")
    assert d_lit <= max(10 * floor, 1e-13 * hmax), (d_lit / hmax, floor / hmax)
    assert d_back <= 1e-8 * hmax   # (the default path again: its element blocks start from the previous assembly's basis, equal to rounding)


def _run(which, literal):
    """test_gpu_fullsize_oracle.py::_run with the key set before the first step: returns the measured errors"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gen_oracle_fullsize as gen
    from thinshelllab_amd.engine.analytic_grad_single import Grad
    from thinshelllab_amd.engine.geometry import projection_query
    path = os.path.join(HERE, "golden", f"oracle_{which}.npz")
    G = np.load(path)
    steps = int(G["stats"].shape[0])
    if which == "cfg4":
        os.environ["TSL_GOLDEN_STEPS"] = str(steps)
    s, drive, steps_b = gen.build(which, device="cuda:0")
    assert steps_b == steps
    gen.apply_ripple(s)
    sel = G["sample_idx"]
    s.spd_literal = literal
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("cg_tol", 1e-10)
    T = steps + 1
    n_part = s.gripper.n_part
    g = Grad(s, T, n_part); g.init_mass(s)
    g.copy_pos(s, 0)
    err = {}
    for f in range(1, steps + 1):
        s.action(f, *drive(f, n_part))
        st = s.time_step(projection_query, f)
        g.copy_pos(s, f)
        nc_o, newton_o = int(G["stats"][f - 1, 0]), int(G["stats"][f - 1, 1])
        assert st["unconverged"] == 0 and st["factorizations"] == st["solves"] > 0, st
        assert st["nc"] == nc_o, (which, literal, f, st["nc"], nc_o)
        assert st["newton_iters"] == newton_o, (which, literal, f, st["newton_iters"], newton_o)
        err[f"x{f}"] = (float(np.abs(s.pos.to_numpy()[sel] - G["pos_buffer_sample"][f]).max()), newton_o >= 50)
    g.pos_grad.t.zero_(); g.angleref_grad.t.zero_()
    if which == "cfg3":
        g.get_loss_fold(s, 1.0, -1.0, rows=s.fold_rows())
    else:
        g.get_loss_balance(s)
    g.transfer_grad(T - 1, s, projection_query)
    ls = g.last_stats
    assert ls["flag"] == 0 and ls["method"] == 4, ls
    pg = g.pos_grad.to_numpy()[T - 2][sel]
    err["pos_grad"] = float(np.abs(pg - G["pos_grad_prev_sample"]).max() / float(G["pos_grad_prev_absmax"]))
    gg = g.gripper_grad.to_numpy()[:T, :n_part]
    ggo = G["gripper_grad"]
    if np.abs(ggo[T - 1]).max() > 0:
        err["gripper_grad"] = float(np.abs(gg[T - 1] - ggo[T - 1]).max() / np.abs(ggo[T - 1]).max())
    else:
        err["gripper_grad"] = float(np.abs(gg[T - 1]).max())
    tz = s.tmp_z_frozen.to_numpy().reshape(-1, 3)[sel]
    tzo = G["tmp_z_frozen_sample"]
    if tzo.shape == tz.shape and np.abs(tzo).max() > 0:
        err["tmp_z_frozen"] = float(np.abs(tz - tzo).max() / np.abs(tzo).max())
    if which == "cfg3" and float(G["angleref_grad_prev_absmax"]) > 0:
        ag = g.angleref_grad.to_numpy().reshape(T, -1)[T - 2, ::7]
        err["angleref_grad"] = float(np.abs(ag - G["angleref_grad_prev_sample"]).max() / float(G["angleref_grad_prev_absmax"]))
    s._close_ctx()
    return err


# bounds of the literal mode, measured values rounded up at most 3x and never looser than test_gpu_fullsize_oracle.py's (x<f>: positions in m after step f,
# gradients relative to the oracle's largest entry).  Measured on the MI355X, literal (default mode in brackets):
#   cfg4  x1 3.6e-12 (1.1e-10), x2 capped 1.3e-7 (1.7e-7), pos_grad 9.2e-6 (5.2e-5), gripper_grad 1.2e-3 (9.9e-4), tmp_z_frozen 1.5e-3 (1.3e-3)
#   cfg3  x1 capped 4.2e-9 (6.2e-11), x2 capped 3.6e-9 (9.1e-11), pos_grad 1.6e-3 (2.4e-4), gripper_grad 2.6e-4 (4.1e-5), tmp_z_frozen 1.3e-2 (2.1e-3),
#         angleref_grad 2.4e-5 (3.7e-6)
# The projector explains part of cfg4's gap and none of cfg3's: behind capped steps the reference's projector, whose thresholds are
# absolute and whose sweeps stop unconverged, passes the rounding differences of the two assemblies on more strongly than the converged eigen-clamp does.
# cfg3's pos_grad and tmp_z_frozen lie above the default mode's absolute bounds (1e-3, 1e-2); they are held to 10x the default mode's error of the same run.
_BOUND = {"cfg4": {"x1": 1e-11, "x2": 4e-7, "pos_grad": 2.5e-5, "gripper_grad": 3e-3, "tmp_z_frozen": 4e-3},
          "cfg3": {"x1": 1.2e-8, "x2": 1e-8, "gripper_grad": 7.5e-4, "angleref_grad": 7e-5}}
_VS_DEFAULT = {"cfg3": ("pos_grad", "tmp_z_frozen")}


@pytest.mark.parametrize("which", ["cfg3", "cfg4"])
def test_literal_fullsize_rollout_vs_oracle_fixture(which):
    lit = _run(which, True)
    dflt = _run(which, False)
    for k in lit:
        if k.startswith("x"):
            print(f"\n{which} step {k[1:]}{' (capped)' if lit[k][1] else ''}: max |x_gpu - x_oracle| literal {lit[k][0]:.2e} m, default {dflt[k][0]:.2e} m", end="")
        else:
            print(f"\n{which} {k}: rel literal {lit[k]:.2e}, default {dflt[k]:.2e}", end="")
    print()
    assert set(lit) == set(_BOUND[which]) | set(_VS_DEFAULT.get(which, ())), sorted(lit)
    for k, b in _BOUND[which].items():
        v = lit[k][0] if k.startswith("x") else lit[k]
        assert v <= b, (which, k, v, b)
    for k in _VS_DEFAULT.get(which, ()):
        assert lit[k] <= 10 * dflt[k], (which, k, lit[k], dflt[k])


def test_literal_rollouts_deterministic():
    """two literal-mode rollouts of a contact scene on the direct path give the same bits"""
    import test_gpu_scenes as tgs
    from thinshelllab_amd.engine.geometry import projection_query
    out = []
    for _ in range(2):
        s = tgs._scene("balancing")
        s.set_spd_literal(True)
        ctx = s._ensure_ctx()
        ctx.set_param("direct", 1)
        n_part = s.gripper.n_part
        xs, sts = [], []
        for f in range(1, 4):
            dpos = np.zeros((n_part, 3)); drot = np.zeros((n_part, 3))
            dpos[:, 2] = 5e-5
            s.action(f, dpos, drot)
            st = s.time_step(projection_query, f)
            xs.append(s.pos.to_numpy().copy()); sts.append((st["nc"], st["newton_iters"], st["energy"]))
        out.append((xs, sts))
        s._close_ctx()
    assert max(st[0] for st in out[0][1]) > 0, "no contact in the rollout"
    assert out[0][1] == out[1][1]
    for a, b in zip(out[0][0], out[1][0]):
        assert np.array_equal(a, b)


def test_literal_group_member_matches_single_scene():
    """a scene-group member with the key set is bit-identical to its single-scene literal run (members assemble on their own contexts; the second
    member keeps the default projector)"""
    import gc
    import test_gpu_group as tgg
    from thinshelllab_amd.engine.geometry import projection_query
    from thinshelllab_amd.scene_group import SceneGroup
    specs = [("balancing", 48, 1.0, True), ("balancing", 48, 1.3, False)]
    T = 4

    def make():
        sc = []
        for name, grid, amp, lit in specs:
            s = tgg._make(name, grid, amp)
            s.set_spd_literal(lit)
            sc.append(s)
        return sc
    single = make()
    res_single = []
    for s in single:
        xs = []
        for f in range(1, T):
            tgg._drive(s, f)
            st = s.time_step(projection_query, f)
            xs.append((s.pos.to_numpy().copy(), st["nc"], st["newton_iters"]))
        res_single.append(xs)
    del single
    gc.collect()
    group = make()
    G = SceneGroup(group)
    res_group = [[] for _ in group]
    for f in range(1, T):
        for s in group:
            tgg._drive(s, f)
        sts = G.time_step(projection_query, f)
        for i, s in enumerate(group):
            res_group[i].append((s.pos.to_numpy().copy(), sts[i]["nc"], sts[i]["newton_iters"]))
    G.close()
    assert max(r[1] for r in res_single[0]) > 0, "no contact in the rollout"
    for i in range(len(specs)):
        for a, b in zip(res_single[i], res_group[i]):
            assert a[1:] == b[1:] and np.array_equal(a[0], b[0]), (i, a[1:], b[1:], np.abs(a[0] - b[0]).max())
    # the key really changed the trajectory of the first member: the same drive without it differs
    s = tgg._make(*specs[0][:3])
    for f in range(1, T):
        tgg._drive(s, f)
        s.time_step(projection_query, f)
    assert not np.array_equal(s.pos.to_numpy(), res_single[0][-1][0])
