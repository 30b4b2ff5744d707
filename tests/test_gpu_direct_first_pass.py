"""The multifrontal LU's FIRST application of its factors, measured against a long-double residual on the host (tests/berr.py).

Every other direct-solve test checks the answer after iterative refinement, which converges as long as the factors are roughly right: a
factor wrong by 1e-4 relative still refines to 1e-12 in three passes.  Here "cg_tol" = 1 and "direct_berr" = 0 make the solve accept its
first pass whenever |r| <= |b|; iters == 1 and exactly one more application of the factors prove that the returned x is the unrefined
(LU)^-1 b (eager sweep and look-ahead at their defaults).  Its normwise backward error |b - Hx| / (|H|_inf |x| + |b|) -- the engine's own
definition, on the FULL operator of operator_csr() -- must be that of a backward-stable solve.

Bound: normwise <= 1e-14 on operators without perturbed pivots (the engine measures 1e-17..1e-16 on cfg4).  Largest values measured on the
MI355X are given per case in the docstrings."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import berr
from helpers import rel_err
from test_direct_plan import FIRST_PASS_SHAPES, check_plan_shape, drape_pattern, dsref_lib, plan_fronts

pytestmark = pytest.mark.gpu

NW_BOUND = 1e-14
CG_TOL, DIRECT_BERR = 1e-10, 1e-12      # the engine's defaults, restored after every first pass


class BoundMissed(AssertionError):
    """the one failure the strict xfails below expect (raises=): a recorded finding.  Every other assertion of those tests -- the ceilings at the
    measured values, the plan shape, iters == 1 -- fails them as usual."""


def _drape(N, M, amp, seed=0):
    from thinshelllab_amd.task_scene.Scene_drape import Scene
    s = Scene(cloth_size=0.1 / 15 * N, N=N, M=M, Kb=100.0, k_angle=3.14)
    s.init_all()
    rng = np.random.default_rng(seed)
    x = s.pos.to_numpy()
    x += rng.normal(0, amp, x.shape)
    s.pos.from_numpy(x)
    s.prev_pos.from_numpy(x)
    return s


def _log(case, **kv):
    print("FIRSTPASS " + case + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def first_pass(ctx, b):
    """x = (LU)^-1 b, unrefined: the solve accepts its first pass (|r| <= |b|), one application of the factors"""
    ctx.set_param("cg_tol", 1.0); ctx.set_param("direct_berr", 0.0)
    a0 = ctx.direct_info()["applications"]
    try:
        x, st = ctx.solve(b.clone())
    finally:
        ctx.set_param("cg_tol", CG_TOL); ctx.set_param("direct_berr", DIRECT_BERR)
    info = ctx.direct_info()
    assert st["method"] == 4 and st["iters"] == 1 and st["flag"] == 0, st
    assert info["applications"] - a0 == 1, (a0, info)
    return x.cpu().numpy(), st, info


def _errs(H, x, b):
    b = b.cpu().numpy() if torch.is_tensor(b) else b
    return berr.normwise_berr(H, x, b), berr.componentwise_berr(H, x, b)


def _scene_plan(ctx, N, M, leaf):
    """the engine's pattern is the grid's clique pattern, and the plan on it holds the shape the case claims (ds_ref: the same direct_plan.hpp)"""
    rp, col, _ = ctx.matrix()
    NV, rp0, col0 = drape_pattern(N, M)
    assert np.array_equal(rp, rp0) and np.array_equal(col, col0)
    F = plan_fronts(dsref_lib(), NV, rp, col, [0, N, M], leaf)
    check_plan_shape(F, FIRST_PASS_SHAPES[(N, M, leaf)])
    return F


def _cpu_plan_solve(ctx, N, M, leaf, b):
    """the same multifrontal plan executed with plain CPU loops in float64 (tests/native/ds_ref.cpp: scalar Gauss-Jordan, no pivoting)"""
    import ctypes as C
    rp, col, vals = ctx.matrix()
    NV = len(rp) - 1
    g = np.array([0, N, M], np.int32); bl = np.zeros(2, np.int32)
    x = np.zeros(3 * NV); st = np.zeros(8); b = np.ascontiguousarray(b, np.float64); vals = np.ascontiguousarray(vals)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert dsref_lib().dsref_solve(NV, P(rp), P(col), P(vals), 1, P(g), 0, P(bl), 0, None, None, leaf, P(b), P(x), P(st)) == 0
    return x


# ---- a. shapes at the kernels' edges ----------------------------------------------------------------------------------------------------
def _edge_case(N, M, leaf, spd):
    s = _drape(N, M, 5e-5 if spd else 2e-4, seed=N + M)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", leaf)
    if spd:
        s.compute_residual_and_Hessian(spd=True)
        b = s.F.to_torch().clone()
    else:
        s.compute_Hessian(spd=False)
        b = torch.as_tensor(np.random.default_rng(3).normal(size=s.tot_NV * 3), device=s.device)
        b = b * torch.as_tensor(s.frozen.to_numpy().reshape(-1) == 0, device=s.device)
    F = _scene_plan(ctx, N, M, leaf)
    x, st, info = first_pass(ctx, b)
    assert info["supernodes"] == len(F) and info["levels"] == F[:, 4].max() + 1, (info, len(F))   # the engine's plan is the one checked
    H = ctx.operator_csr()
    nw, cw = _errs(H, x, b)
    nw_cpu = berr.normwise_berr(H, _cpu_plan_solve(ctx, N, M, leaf, b.cpu().numpy()), b.cpu().numpy())
    _log(f"a:{N}x{M}/leaf{leaf}/{'spd' if spd else 'indef'}", nw=nw, cw=cw, nw_cpu_plan=nw_cpu, rel=st["rel_residual"], perturbed=int(info["perturbed_pivots"]),
         guarded=int(ctx.direct_counters()["tiles_guarded"]), fronts=int(info["supernodes"]))
    assert info["perturbed_pivots"] == 0, info
    return nw, cw, nw_cpu


@pytest.mark.parametrize("N,M,leaf", sorted(FIRST_PASS_SHAPES))
def test_first_pass_at_kernel_edges(N, M, leaf):
    """Plans whose fronts have p = 32k - 1, 32k, 32k + 1, b = 32k - 1, 32k + 1, the root (b = 0), padded pivot blocks on both sides of 128 and 512, one front
    (FIRST_PASS_SHAPES, checked on the plan itself), projected (spd) operator.  Largest normwise first-pass error measured on the MI355X:
    2.1e-15 (the single front of 1344 pivots), 1.8e-16 on the others."""
    nw, cw, nw_cpu = _edge_case(N, M, leaf, True)
    assert nw <= NW_BOUND, (N, M, leaf, nw, cw)


# measured on the MI355X (normwise first pass / the same plan run with plain CPU loops, tests/native/ds_ref.cpp): 20 x 20 one front 4.6e-16 /
# 2.2e-16; 100 x 60 7.8e-14 / 3.0e-14; 33 x 70 1.9e-13 / 1.8e-15; 64 x 64 8.8e-13 / 5.2e-14 -- no pivot perturbed, no tile guarded
_INDEF_ABOVE = pytest.mark.xfail(strict=True, raises=BoundMissed, reason="un-projected indefinite operator: first pass above 1e-14 (DESIGN.md 9d)")
INDEF_CEILING = 1e-11      # 11x the largest value measured: a regression beyond it fails the test, xfail or not


@pytest.mark.parametrize("N,M,leaf", [pytest.param(*k, marks=() if k == (20, 20, 500) else _INDEF_ABOVE) for k in sorted(FIRST_PASS_SHAPES)])
def test_first_pass_at_kernel_edges_indefinite(N, M, leaf):
    """The same plans on the un-projected, indefinite operator of a strongly perturbed drape (the adjoint's systems), same bound.  Three of the
    four plans land above it without a perturbed pivot -- 2.6x to 100x above the plain-loop CPU run of the same plan, which is itself above
    1e-14 on two of them.  LU without pivoting grows on these operators; why the GPU grows more than scalar Gauss-Jordan is not measured yet
    (the 4 x 4 cofactor block steps are the suspect).  Recorded as a finding: strict xfail on the 1e-14 bound only (BoundMissed), a plain
    failure above INDEF_CEILING."""
    nw, cw, nw_cpu = _edge_case(N, M, leaf, False)
    assert nw <= INDEF_CEILING, (N, M, leaf, nw, nw_cpu, cw)
    if nw > NW_BOUND:
        raise BoundMissed((N, M, leaf, nw, nw_cpu, cw))


# ---- b. bodies and contact --------------------------------------------------------------------------------------------------------------
def _balancing_after_two_steps():
    from thinshelllab_amd.engine.geometry import projection_query
    from thinshelllab_amd.task_scene.Scene_balancing import Scene
    s = Scene(cloth_size=0.06, cloth_N=48, cloth_M=48)
    s.init_all()
    s.mu_cloth_elastic[None] = 5.0
    s.prev_pos.copy_from(s.pos)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1)
    n_part = s.gripper.n_part
    dpos = np.zeros((n_part, 3)); drot = np.zeros((n_part, 3)); dpos[:, 2] = [1e-4, -1e-4][:n_part]
    for f in range(1, 3):
        s.action(f, dpos, drot)
        st = s.time_step(projection_query, f)
        assert st["unconverged"] == 0, st
    assert st["nc"] > 0
    projection_query(s)
    return s, ctx


def test_first_pass_with_bodies_and_contact():
    """balancing 48 x 48 after two driven steps (FEM bodies as dense supernodes, contact cliques in the tree): forward (projected) and adjoint
    (un-projected) operator.  Normwise bound as everywhere; componentwise bounded as MEASURED only (an LU without row exchanges is not
    componentwise stable next to contact entries of 1e13): largest measured values in the pull request table.
    f: the backward error the engine reports for the refined solve of the same systems ("cg_tol" 1e-18: refinement to the attainable
    accuracy, which reports it) is never below half of the host's value on the full operator."""
    s, ctx = _balancing_after_two_steps()
    free = torch.as_tensor(s.frozen.to_numpy().reshape(-1) == 0, device=s.device)
    for spd in (True, False):
        if spd:
            s.compute_residual_and_Hessian(spd=True)
            b = s.F.to_torch().clone()
        else:
            s.compute_Hessian(spd=False)
            b = torch.as_tensor(np.random.default_rng(5).normal(size=s.tot_NV * 3), device=s.device) * free
        H = ctx.operator_csr()
        x, st, info = first_pass(ctx, b)
        nw, cw = _errs(H, x, b)
        _log(f"b:balancing48/{'forward' if spd else 'adjoint'}", nw=nw, cw=cw, rel=st["rel_residual"], perturbed=int(info["perturbed_pivots"]),
             guarded=int(ctx.direct_counters()["tiles_guarded"]))
        assert info["perturbed_pivots"] == 0, info
        assert nw <= NW_BOUND, (spd, nw, cw)
        assert cw <= 1e-11, (spd, nw, cw)       # measured 9.9e-14 (forward) and 3.1e-13 (adjoint); normwise 8.0e-17 / 8.4e-17
        # f: the reported backward error of the refined answer
        ctx.set_param("cg_tol", 1e-18)
        xr, str_ = ctx.solve(b.clone())
        ctx.set_param("cg_tol", CG_TOL)
        hb = berr.normwise_berr(H, xr.cpu().numpy(), b.cpu().numpy())
        _log(f"f:balancing48/{'forward' if spd else 'adjoint'}", reported=str_["backward_error"], host=hb, iters=str_["iters"])
        assert str_["backward_error"] > 0 and str_["backward_error"] >= 0.5 * hb, (str_, hb)


# ---- c. every factorisation path on one shape ---------------------------------------------------------------------------------------
PATHS = [
    dict(),                                                                                     # defaults: dataflow chains, LDS kernel, look-ahead 103
    dict(direct_flow=0, direct_lookahead=0),                                                    # block-step launches, nothing on the side stream
    dict(direct_flow=0, direct_small_rounds=1),                                                 # LDS kernel skipped for the leaf batch
    dict(direct_g32_below=0, direct_gemv_wide_below=0),                                         # G in 64 x 64 tiles, narrow sweeps everywhere
    dict(direct_g32_below=1 << 30, direct_gemv_wide_below=1 << 30),                             # G in 32 x 32 tiles, wide sweeps everywhere
    dict(direct_flow=3, direct_small_rounds=1, direct_lookahead=0),
]


def test_first_pass_on_every_factorisation_path():
    """200 x 200 drape, leaves of 32 vertices (several fronts per upper level; a leaf batch of 583 fronts of 96 pivots that the LDS kernel takes
    in two rounds of the chip and leaves to the block-step launches at one): each path gets the first-pass bound itself, not only bit
    equality with its neighbour (a bug in shared code -- the tile inversion, the GEMM epilogue, the padding -- passes every equality test)"""
    s = _drape(200, 200, 5e-5, seed=5)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", 32)
    defaults = dict(direct_flow=3, direct_small_rounds=2, direct_g32_below=1100, direct_gemv_wide_below=300, direct_lookahead=103)
    flow_seen, lds = False, []
    for path in PATHS:
        for k, v in {**defaults, **path}.items():
            ctx.set_param(k, v)
        s.compute_residual_and_Hessian(spd=True)
        b = s.F.to_torch().clone()
        n0 = ctx.direct_counters()["flow_launches"]
        x, st, info = first_pass(ctx, b)
        flow_seen |= ctx.direct_counters()["flow_launches"] > n0
        nw, cw = _errs(ctx.operator_csr(), x, b)
        # batches this factorisation ran in the LDS kernel / on the block-step launches (the replays of tsl_bench_direct pick the same kernel
        # per batch as direct_factor; they overwrite the factors, which the next path forms again)
        lds.append((int(ctx.bench_direct(3, 1)["launches"]), int(ctx.bench_direct(0, 1)["launches"])))
        _log("c:" + (",".join(f"{k}={v}" for k, v in path.items()) or "defaults"), nw=nw, cw=cw, perturbed=int(info["perturbed_pivots"]),
             lds_batches=lds[-1][0], block_step_batches=lds[-1][1])
        assert info["perturbed_pivots"] == 0 and nw <= NW_BOUND, (path, nw, cw)
    assert flow_seen, "no dataflow launch ran (the device's token is held by a context that is still alive?)"
    # "direct_flow" 0: the LDS kernel takes batches at "direct_small_rounds" 2 and fewer of them at 1 (those go to the block-step launches)
    assert lds[1][0] > 0 and lds[2][0] < lds[1][0] and lds[2][1] > lds[1][1], lds


# ---- d. non-symmetric and badly scaled values (tsl_matrix_import) --------------------------------------------------------------------
def _dominant_nonsymmetric(rp, col, rng):
    """values in the pattern (rp, col): every entry independent (H_ij and H_ji drawn separately), diagonal 1.5..3 x the rest of its row"""
    vals = rng.uniform(-1.0, 1.0, (len(col), 3, 3)) * 10.0 ** rng.uniform(-2, 0, (len(col), 1, 1))
    NV = len(rp) - 1
    rowsum = np.zeros(3 * NV)
    for v in range(NV):
        for q in range(rp[v], rp[v + 1]):
            blk = vals[q].copy()
            if col[q] == v:
                np.fill_diagonal(blk, 0.0)
            rowsum[3 * v:3 * v + 3] += np.abs(blk).sum(axis=1)
    for v in range(NV):
        q = rp[v] + int(np.nonzero(col[rp[v]:rp[v + 1]] == v)[0][0])
        for r in range(3):
            vals[q, r, r] = rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 3.0) * (rowsum[3 * v + r] + 1e-3)
    return vals


def _scaled(rp, col, vals, d1, d2):
    out = vals.copy()
    for v in range(len(rp) - 1):
        for q in range(rp[v], rp[v + 1]):
            out[q] = d1[3 * v:3 * v + 3, None] * vals[q] * d2[None, 3 * col[q]:3 * col[q] + 3]
    return out


def _nonsymmetric_system():
    s = _drape(40, 40, 5e-5, seed=2)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", 16)
    s.compute_residual_and_Hessian(spd=True)
    rp, col, _ = ctx.matrix()
    rng = np.random.default_rng(11)
    vals = _dominant_nonsymmetric(rp, col, rng)
    ctx.matrix_import(vals)
    H = ctx.matrix_csr()
    off = H - sp.diags(H.diagonal())
    assert abs(H - H.T).max() > 0.5 * abs(off).max()
    b = torch.as_tensor(rng.standard_normal(H.shape[0]), device=s.device)
    return s, ctx, rp, col, vals, H, b, rng


def test_first_pass_nonsymmetric_values():
    """Strictly diagonally dominant, deliberately NON-symmetric values in a real scene's pattern and plan (40 x 40 drape, leaves of 16: H_ij and
    H_ji drawn independently): a kernel that used F12 where it needs F21^T fails here.  LU without pivoting is stable on such matrices.
    Measured on the MI355X: normwise 3.8e-17, componentwise 6.7e-16."""
    s, ctx, rp, col, vals, H, b, rng = _nonsymmetric_system()
    x, st, info = first_pass(ctx, b)
    nw, cw = _errs(H, x, b)
    _log("d:nonsymmetric", nw=nw, cw=cw, perturbed=int(info["perturbed_pivots"]), guarded=int(ctx.direct_counters()["tiles_guarded"]))
    assert info["perturbed_pivots"] == 0 and nw <= NW_BOUND, (nw, cw)
    assert cw <= 1e-13, cw


@pytest.mark.xfail(strict=True, raises=BoundMissed, reason="static-pivot rule not invariant under row / column scaling: 172 pivots perturbed at 2^-10..2^43 (DESIGN.md 9d)")
def test_first_pass_scaled_by_powers_of_two():
    """The non-symmetric system above with rows and columns scaled by independent powers of two in 2^-10 .. 2^43 (the range of a frozen dof next
    to a contact entry): every operation scales exactly, so the solution must be D2^-1 times the unscaled one to 1e-13 per component, no pivot
    perturbed, componentwise bound on the scaled system.  An absolute or tile-relative threshold hidden in a kernel shows up here -- and does:
    measured on the MI355X, 172 perturbed pivots, 123 guarded tiles, solutions 17x apart (the floor tmax x 1e-20 of the guarded form and the
    row-scaled test of the cofactor path).  Strict, and on these three conditions only (BoundMissed): the unscaled first pass, the scaled first
    pass's normwise error and the refined solve of the scaled system are asserted as usual."""
    s, ctx, rp, col, vals, H, b, rng = _nonsymmetric_system()
    x, st, info = first_pass(ctx, b)
    assert info["perturbed_pivots"] == 0 and berr.normwise_berr(H, x, b.cpu().numpy()) <= NW_BOUND
    n = H.shape[0]
    d1 = 2.0 ** rng.integers(-10, 44, n).astype(float); d2 = 2.0 ** rng.integers(-10, 44, n).astype(float)
    ctx.matrix_import(_scaled(rp, col, vals, d1, d2))
    Hs = ctx.matrix_csr()
    bs = torch.as_tensor(d1 * b.cpu().numpy(), device=s.device)
    xs, st_s, info_s = first_pass(ctx, bs)
    nws, cws = _errs(Hs, xs, bs)
    dev = np.abs(xs * d2 - x) / np.abs(x)
    perturbed, guarded = int(info_s["perturbed_pivots"]), int(ctx.direct_counters()["tiles_guarded"])
    # the refined solve of the scaled system still meets cg_tol (static pivoting is what refinement repairs)
    xr, st_r = ctx.solve(bs.clone())
    bsn = bs.cpu().numpy()
    rr = float(np.linalg.norm(np.asarray(berr.residual(Hs, xr.cpu().numpy(), bsn), float)) / np.linalg.norm(bsn))
    cwr = berr.componentwise_berr(Hs, xr.cpu().numpy(), bsn)
    _log("d:scaled", nw=nws, cw=cws, perturbed=perturbed, guarded=guarded, max_rel_dev=float(dev.max()), refined_rel=rr, refined_cw=cwr,
         refined_iters=st_r["iters"], refined_flag=st_r["flag"])
    assert nws <= NW_BOUND, nws
    # ceiling, not the goal: the engine's double-precision residual cannot resolve this system's 2^106 spread of entries, and the refined
    # answer it accepts at cg_tol is 1.6e-8 of |b| in long double (measured)
    assert st_r["flag"] == 0 and rr <= 1e-6, (st_r, rr)
    if perturbed != 0 or cws > 1e-13 or dev.max() > 1e-13:
        raise BoundMissed((perturbed, guarded, cws, float(dev.max())))


def test_matrix_import_round_trips():
    """importing matrix() unchanged gives the same bits from tsl_solve as before the import"""
    s = _drape(48, 32, 5e-5, seed=3)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", 32)
    s.compute_residual_and_Hessian(spd=True)
    b = s.F.to_torch().clone()
    x0, st0 = ctx.solve(b.clone())
    rp, col, vals = ctx.matrix()
    f0 = ctx.direct_info()["factorizations"]
    ctx.matrix_import(vals)
    x1, st1 = ctx.solve(b.clone())
    assert ctx.direct_info()["factorizations"] == f0 + 1          # the import made the factors stale
    assert np.array_equal(ctx.matrix()[2], vals)
    assert st0["flag"] == 0 and np.array_equal(x0.cpu().numpy(), x1.cpu().numpy()) and st0["iters"] == st1["iters"]


# ---- e. static pivoting and the guarded form ----------------------------------------------------------------------------------------
def test_static_pivoting_positive_control():
    """"direct_piv_tol" 0.5 perturbs healthy pivots: the first pass misses the bound by orders of magnitude (the test sees a wrong factor);
    with the default tolerance back the refined solve meets cg_tol and agrees with x_ref"""
    s = _drape(40, 40, 5e-5, seed=4)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", 16)
    ctx.set_param("direct_piv_tol", 0.5)
    s.compute_residual_and_Hessian(spd=True)
    b = s.F.to_torch().clone()
    H = ctx.operator_csr()
    x, st, info = first_pass(ctx, b)
    nw, cw = _errs(H, x, b)
    _log("e:piv_tol=0.5", nw=nw, cw=cw, perturbed=int(info["perturbed_pivots"]), guarded=int(ctx.direct_counters()["tiles_guarded"]))
    assert info["perturbed_pivots"] > 0 and nw > 1e3 * NW_BOUND, (info, nw)
    ctx.set_param("direct_piv_tol", 1e-11)
    s.compute_residual_and_Hessian(spd=True)
    xr, st = ctx.solve(b.clone())
    bn = b.cpu().numpy()
    assert st["flag"] == 0 and np.linalg.norm(np.asarray(berr.residual(H, xr.cpu().numpy(), bn), float)) <= CG_TOL * np.linalg.norm(bn)
    assert rel_err(xr.cpu().numpy(), berr.x_ref(H, bn)) < 1e-9


def _leaf_fronts(ctx, N, M, leaf):
    rp, col, vals = ctx.matrix()
    NV, _, _ = drape_pattern(N, M)
    F = plan_fronts(dsref_lib(), NV, rp, col, [0, N, M], leaf)
    leaves = F[(F[:, 5] == 0) & (F[:, 0] >= 9)]
    return rp, col, vals, leaves


def _block(rp, col, r, c):
    hit = np.nonzero(col[rp[r]:rp[r + 1]] == c)[0]
    return rp[r] + int(hit[0]) if len(hit) else -1


def _plant(rp, col, vals, v, blk, cut=()):
    """vertex v's diagonal block := blk; the blocks between v and every vertex of `cut` := 0 (both directions)"""
    vals[_block(rp, col, v, v)] = blk
    for u in cut:
        for a, c in ((v, u), (u, v)):
            q = _block(rp, col, a, c)
            if q >= 0:
                vals[q] = 0.0


def test_near_singular_coupling_is_guarded_and_refined():
    """A near-singular pair of dofs [[1, 1], [1, 1 + 1e-12]] (times the entry's scale) at the head of a leaf front's pivot block: the cofactor
    path's determinant cancels, the tile goes through the guarded form, the Schur pivot (1e-12 of its diagonal) is perturbed.  The default solve
    must NOT accept that first pass on the backward-error rule and must still end with a host backward error <= 1e-12.  In the same tile, the
    next 4 x 4 pivot block opens with an exact zero ([0 a; a 0], decoupled from the pair): the guarded form inverts it exactly -- ONE perturbed
    pivot, not two."""
    N = M = 40; leaf = 64
    s = _drape(N, M, 5e-5, seed=6)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", leaf)
    s.compute_residual_and_Hessian(spd=True)
    rp, col, vals, leaves = _leaf_fronts(ctx, N, M, leaf)
    v1, v2 = int(leaves[0, 6]), int(leaves[0, 10])
    sc = float(np.abs(vals[_block(rp, col, v1, v1)]).max())
    _plant(rp, col, vals, v1, sc * np.array([[1, 1, 0], [1, 1 + 1e-12, 0], [0, 0, 1.0]]), cut=(v2,))      # dofs 0, 1: pivot block 0
    _plant(rp, col, vals, v2, sc * np.array([[1.0, 0, 0], [0, 0, 1], [0, 1, 0]]))                          # dofs 4, 5: pivot block 1 opens with 0
    ctx.matrix_import(vals)
    H = ctx.operator_csr()
    b = s.F.to_torch().clone()
    bn = b.cpu().numpy()
    a0 = ctx.direct_info()["applications"]
    x, st = ctx.solve(b.clone())
    info, k = ctx.direct_info(), ctx.direct_counters()
    hb = berr.normwise_berr(H, x.cpu().numpy(), bn)
    _log("e:near-singular", perturbed=int(info["perturbed_pivots"]), guarded=int(k["tiles_guarded"]), iters=st["iters"],
         applications=int(info["applications"] - a0), host_berr=hb, reported=st["backward_error"])
    assert info["perturbed_pivots"] == 1 and k["tiles_guarded"] >= 1, (info, k)
    assert st["iters"] > 1, st
    assert st["flag"] == 0 and hb <= 1e-12, (st, hb)
    if st["backward_error"] > 0:
        assert st["backward_error"] >= 0.5 * hb, (st, hb)


def test_zero_leading_entry_is_inverted_exactly():
    """[0 a; a 0] with a healthy determinant at the head of a leaf front's pivot block (dofs 0, 1): inverted exactly by the cofactor path, no
    pivot perturbed, first-pass bound.  The cofactor path's static-pivot rule compares the inverse with the row's own diagonal: a zero
    diagonal does not send the tile to the guarded form, so tiles_guarded stays 0 (measured) -- not > 0.  The guarded form's exact inversion
    of such a block is covered by test_near_singular_coupling_is_guarded_and_refined (one perturbed pivot, not two)."""
    N = M = 40; leaf = 64
    s = _drape(N, M, 5e-5, seed=7)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", leaf)
    s.compute_residual_and_Hessian(spd=True)
    rp, col, vals, leaves = _leaf_fronts(ctx, N, M, leaf)
    for f in leaves[:4]:
        v = int(f[6])
        sc = float(np.abs(vals[_block(rp, col, v, v)]).max())
        _plant(rp, col, vals, v, sc * np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1.0]]))
    ctx.matrix_import(vals)
    H = ctx.operator_csr()
    b = s.F.to_torch().clone()
    x, st, info = first_pass(ctx, b)
    nw, cw = _errs(H, x, b)
    k = ctx.direct_counters()
    _log("e:zero-leading", nw=nw, cw=cw, perturbed=int(info["perturbed_pivots"]), guarded=int(k["tiles_guarded"]))
    assert info["perturbed_pivots"] == 0 and k["tiles_guarded"] == 0 and nw <= NW_BOUND, (info, k, nw, cw)


# ---- f. the backward error the engine reports --------------------------------------------------------------------------------------
def _norm_used(st, x, b):
    """|H|_inf the engine divided by: backward_error = |r| / (anorm |x| + |b|) and rel_residual = |r| / |b| come from the same pass of the
    refinement (direct_refine / ir_pass_verdict), so anorm = (rel_residual |b| / backward_error - |b|) / |x|"""
    nb, nx = float(np.linalg.norm(b)), float(np.linalg.norm(x))
    return (st["rel_residual"] * nb / st["backward_error"] - nb) / nx


def test_reported_backward_error_follows_the_operator_between_assemblies():
    """|H|_inf, the yardstick of the reported backward error, is cached across factorisations.  Two tsl_assemble calls on one context without a
    set_param in between -- the first on a drape stretched to eight times its size, the second at rest -- and |vals|_inf halves (measured 1.0e7
    -> 5.1e6).  The norm each solve divided by is recovered from its own statistics and must be |H|_inf of the operator in place, to 1e-10:
    a norm kept from the first assembly is 1.97x off.  And the reported backward error is never below half of the host's value (a stale,
    larger norm makes it too small and lets a first pass skip refinement wrongly)."""
    s = _drape(40, 40, 5e-5, seed=8)
    ctx = s._ensure_ctx()
    ctx.set_param("direct", 1); ctx.set_param("direct_leaf", 16)
    ctx.set_param("cg_tol", 1e-18)             # refinement to the attainable accuracy: the solve reports its backward error
    x_rest = s.pos.to_numpy().copy()
    c = x_rest.mean(axis=0)
    x_big = c + 8.0 * (x_rest - c)
    norms, out = [], []
    try:
        for pos in (x_big, x_rest):
            s.pos.from_numpy(pos); s.prev_pos.from_numpy(pos)
            s.compute_residual_and_Hessian(spd=True)
            b = s.F.to_torch().clone()
            assert torch.any(b != 0)
            H = ctx.operator_csr()
            assert (H - ctx.matrix_csr()).nnz == 0          # no contact blocks: the static part the norm covers is the whole operator
            norms.append(float(berr.inf_norm(H)))
            x, st = ctx.solve(b.clone())
            xn, bn = x.cpu().numpy(), b.cpu().numpy()
            hb = berr.normwise_berr(H, xn, bn)
            used = _norm_used(st, xn, bn) if st["backward_error"] > 0 else float("nan")
            out.append((st, hb, used))
            _log("f:stale-norm", anorm=norms[-1], anorm_used=used, reported=st["backward_error"], host=hb, iters=st["iters"])
    finally:
        ctx.set_param("cg_tol", CG_TOL)
    assert norms[0] > 1.8 * norms[1], norms
    for (st, hb, used), nrm in zip(out, norms):
        assert st["method"] == 4 and st["backward_error"] > 0, st
        assert abs(used - nrm) <= 1e-10 * nrm, (used, nrm, norms)
        assert st["backward_error"] >= 0.5 * hb, (st, hb)
