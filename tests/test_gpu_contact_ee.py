"""Edge-edge contact, the context key "contact_ee" (include/tsl_hip.h, csrc/k_contact.hpp).  The reference has vertex-triangle contact only,
so the new term is checked against a NumPy restatement (tests/ee_numpy.py), brute-force detection and finite differences, not against the
oracle.  The scene is two diamond-section bars crossing ridge over ridge (no vertex over the other ridge): vertex-triangle contact sees
nothing there while the ridges pass through each other.

These tests hold the mode as a whole: the key, detection against a brute-force search, pass-through, rollout differences, solvers, groups.  The kernels
alone -- records, blocks per 3 x 3 sub-block, the 9 -> 12 row map, launch edges, slot offsets, the frozen mask, the reverse step -- are held against an
mpmath restatement at the bound of the other element kernels by tests/test_gpu_ee_elements.py (tests/ee_elements_numpy.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ee_numpy as en  # noqa: E402

pytestmark = pytest.mark.gpu


def _state(sc, x=None):
    x = sc["x"] if x is None else x
    pos = torch.tensor(x, dtype=torch.float64, device="cuda")
    return pos, pos.clone(), torch.zeros_like(pos), torch.zeros(3, dtype=torch.float64, device="cuda")


def _rollout(ctx, sc, T, x0=None):
    pos, prev, vel, ref = _state(sc, x0)
    xs, sts = [pos.cpu().numpy().copy()], []
    for _ in range(1, T):
        st = ctx.step(pos, prev, vel, ref)
        xs.append(pos.cpu().numpy().copy())
        sts.append((st, ctx.contact_counts()))
    return np.array(xs), sts


# ------------------------------------------------------------------------------------------------ off is off
def test_key_defaults_off_and_accepts_0_and_1_only():
    sc = en.bar_scene(gap=2e-4)
    ctx = en.bar_context(sc)
    pos, prev, _, _ = _state(sc)
    ctx.contact_detect(pos, prev)
    assert ctx.contact_counts() == (0, 0)   # qualifying edge pairs exist (below), the default mode does not look for them
    with pytest.raises(Exception):
        ctx.set_param("contact_ee", 2)
    ctx.set_param("contact_ee", 1)
    ctx.contact_detect(pos, prev)
    assert ctx.contact_counts()[0] == 0 and ctx.contact_counts()[1] > 0
    ctx.set_param("contact_ee", 0)
    ctx.contact_detect(pos, prev)
    assert ctx.contact_counts() == (0, 0)


def test_tape_bit_identical_with_key_on_when_nothing_qualifies():
    """the bars 3 mm apart (no qualifying edge pair within the rollout): forward tape and reverse sweep are the same bits with contact_ee 0 and 1.
    (Every task scene has qualifying edge pairs within its first steps -- cloth edges lying across pad and table edges -- so none of them serves.)"""
    T = 4
    sc = en.bar_scene(gap=3e-3)
    NV = len(sc["x"])
    out = []
    for ee in (0, 1):
        ctx = en.bar_context(sc)
        ctx.set_param("contact_ee", ee)
        xs, sts = _rollout(ctx, sc, T)
        pb = torch.tensor(xs, device="cuda").contiguous()
        pg = torch.zeros_like(pb)
        pg[T - 1] = torch.tensor(np.random.default_rng(3).normal(size=(NV, 3)), device="cuda")
        rb = torch.zeros((T, 3), dtype=torch.float64, device="cuda"); ag = torch.zeros_like(rb)
        tz = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
        for st_ in range(T - 1, 0, -1):
            ctx.adjoint_step(st_, T, pb, pg, rb, ag, tz, 1.0)
        out.append((xs, pg.cpu().numpy(), [c for _, c in sts]))
        ctx.close()
    assert all(c == (0, 0) for c in out[1][2])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------ pass-through
def test_bars_pass_through_without_and_are_held_with_edge_edge_contact():
    T = 24
    sc = en.bar_scene(gap=5e-4)
    res = {}
    for ee in (0, 1):
        ctx = en.bar_context(sc)
        ctx.set_param("contact_ee", ee)
        xs, sts = _rollout(ctx, sc, T)
        res[ee] = ([en.ridge_distance(x, sc) for x in xs], [c for _, c in sts], [st["unconverged"] for st, _ in sts])
        ctx.close()
    d0, c0, _ = res[0]
    first_neg = next(i for i, d in enumerate(d0) if d < 0)   # (StopIteration: the ridges never crossed)
    assert all(c == (0, 0) for c in c0[:first_neg]), "vertex-triangle contact fired before the ridges crossed"
    assert min(d0) < -1e-3
    d1, c1, u1 = res[1]
    assert all(c[0] == 0 for c in c1) and max(c[1] for c in c1) > 0
    assert min(d1) > 0, min(d1)
    assert max(d1[-6:]) - min(d1[-6:]) < 1e-4, d1[-6:]
    assert sum(u1) == 0


# ------------------------------------------------------------------------------------------------ detection
@pytest.mark.parametrize("case", ["crumpled", "coarse", "spanning"])
def test_detection_equals_brute_force(case):
    """crumpled: both bars tangled ridge into ridge at 60 degrees, every vertex displaced at random; coarse: edges (1 cm) longer than grid_h;
    spanning: the crumpled bars with a first descriptor whose query range covers both bodies (the pair is taken once, from it)"""
    coarse = case == "coarse"
    rng = np.random.default_rng(11 if coarse else 7)
    if coarse:
        sc = en.bar_scene(n=6, dx=0.01, w=0.01, gap=-3e-3, angle=np.pi / 3)
        x = sc["x"] + rng.normal(scale=1.5e-3, size=sc["x"].shape)
        eps = 2e-3
    else:
        sc = en.bar_scene(n=16, dx=0.0025, w=0.005, n_up=14, gap=-1.5e-3, angle=np.pi / 3)
        x = sc["x"] + rng.normal(scale=4e-4, size=sc["x"].shape)
        eps = 1e-3
    if case == "spanning":
        sc["pairs"] = [(0, 0, len(x), 0.5)] + sc["pairs"]
    ctx = en.bar_context(sc, eps_contact=eps)
    ctx.set_param("contact_ee", 1)
    pos = torch.tensor(x, device="cuda")
    ctx.contact_detect(pos, pos.clone())
    n_vf, n_ee = ctx.contact_counts()
    cons = ctx.constraints()
    assert len(cons["idx"]) == n_vf + n_ee
    idx_ref, st_ref = en.brute_force(x, sc["faces"], sc["bodies"], sc["pairs"], eps)
    assert n_ee == len(idx_ref) and n_ee >= (5 if coarse else 20), (n_ee, len(idx_ref))
    assert np.array_equal(cons["idx"][n_vf:], idx_ref)
    assert np.abs(cons["w"][n_vf:, :2] - st_ref).max() < 1e-12
    assert np.all(cons["w"][n_vf:, 2] == 0)
    # the record fields at detection (pos = prev = x): dx0, k, mu, n, T
    for i, (idx, st) in enumerate(zip(idx_ref, st_ref)):
        r = en.record(x, x, idx, st, 1000.0, eps, 0.5)
        j = n_vf + i
        assert np.abs(cons["dx0"][j] - r["dx0"]).max() <= 1e-15
        assert abs(cons["k"][j] - r["k"]) <= 1e-12 * abs(r["k"]) and cons["mu"][j] == 0.5
        assert np.abs(cons["n"][j] - r["n"]).max() <= 1e-12 and np.abs(cons["T"][j] - r["T"]).max() <= 1e-12
    # the normal of a slot points to the query edge's side at detection: positive line distance
    for i in range(n_vf, n_vf + n_ee):
        assert en.line_distance(x[cons["idx"][i]]) >= 0
    # same bits on a second detection
    ctx.contact_detect(pos, pos.clone())
    c2 = ctx.constraints()
    for k in cons:
        assert np.array_equal(cons[k], c2[k]), k


# ------------------------------------------------------------------------------------------------ derivatives
def _ee_only_ctx(mu):
    sc = en.bar_scene(gap=4e-4, mu=mu)
    ctx = en.bar_context(sc)
    ctx.set_param("contact_ee", 1)
    x = sc["x"]
    pos = torch.tensor(x, device="cuda")
    ctx.contact_detect(pos, pos.clone())
    n_vf, n_ee = ctx.contact_counts()
    assert n_vf == 0 and n_ee > 0
    # evaluate away from the detection state: the upper bar pressed down and slid (friction slip above eps_v dt)
    x1 = x.copy()
    nl = sc["n_lower"]
    rng = np.random.default_rng(2)
    x1[nl:] += np.array([1.5e-4, -1e-4, -2e-4]) + rng.normal(scale=2e-5, size=x1[nl:].shape)
    return sc, ctx, x, x1


def _grad(ctx, x, prev, spd=False):
    pos = torch.tensor(x, device="cuda"); pv = torch.tensor(prev, device="cuda")
    g = torch.zeros(x.size, dtype=torch.float64, device="cuda")
    ctx.assemble(pos, pv, torch.zeros_like(pos), torch.zeros(3, dtype=torch.float64, device="cuda"), spd=spd, grad=g)
    return g.cpu().numpy()


def _energy(ctx, x, prev):
    pos = torch.tensor(x, device="cuda"); pv = torch.tensor(prev, device="cuda")
    return ctx.energy(pos, pv, torch.zeros_like(pos), torch.zeros(3, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("mu", [0.0, 0.5])
def test_gradient_matches_energy_differences(mu):
    sc, ctx, x, x1 = _ee_only_ctx(mu)
    g = _grad(ctx, x1, x)
    cons = ctx.constraints()
    dofs = sorted({3 * v + a for v in cons["idx"].ravel() for a in range(3) if v >= sc["n_lower"]})   # every free dof of every constraint (frozen rows are zero)
    assert len(dofs) > 0
    h = 1e-7
    for i in dofs:
        xp = x1.copy(); xp.flat[i] += h
        xm = x1.copy(); xm.flat[i] -= h
        fd = (_energy(ctx, xp, x) - _energy(ctx, xm, x)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * np.abs(g[dofs]).max(), (i, fd, g[i])


@pytest.mark.parametrize("mu", [0.0, 0.5])
def test_terms_match_numpy_restatement(mu):
    """contact gradient = gradient with the constraints minus gradient without them; d through the contact energy; blocks (spd 0) against
    differences of the restated gradient; spd 1 blocks positive semidefinite"""
    sc, ctx, x, x1 = _ee_only_ctx(mu)
    cons = ctx.constraints()
    g_with = _grad(ctx, x1, x)
    E_with = _energy(ctx, x1, x)
    ctx.assemble(torch.tensor(x1, device="cuda"), torch.tensor(x, device="cuda"), torch.zeros(x.shape, dtype=torch.float64, device="cuda"),
                 torch.zeros(3, dtype=torch.float64, device="cuda"), spd=False)
    H0 = ctx.contact_blocks(masked=False)
    ctx.assemble(torch.tensor(x1, device="cuda"), torch.tensor(x, device="cuda"), torch.zeros(x.shape, dtype=torch.float64, device="cuda"),
                 torch.zeros(3, dtype=torch.float64, device="cuda"), spd=True)
    H1 = ctx.contact_blocks(masked=False)
    far = x.copy(); far[sc["n_lower"]:, 2] += 0.05
    pf = torch.tensor(far, device="cuda")
    ctx.contact_detect(pf, pf.clone())
    assert ctx.contact_counts() == (0, 0)
    g_c = g_with - _grad(ctx, x1, x)
    E_c = E_with - _energy(ctx, x1, x)
    k_contact, eps, eh = 1000.0, 1e-3, 0.01 * 5e-3
    g_ref = np.zeros_like(g_c)
    E_ref, fr_norm = 0.0, 0.0
    for i, idx in enumerate(cons["idx"]):
        X = x1[idx]
        fn = lambda Z: en.energy_normal(Z, k_contact, eps)
        ff = lambda Z, i=i: en.energy_friction(Z, cons["w"][i], cons["dx0"][i], cons["T"][i], cons["k"][i], eh)
        gn, gf = en.grad_cs(fn, X), en.grad_cs(ff, X)
        fr_norm = max(fr_norm, np.abs(gf).max())
        E_ref += fn(X) + ff(X)
        np.add.at(g_ref, (3 * idx[:, None] + np.arange(3)).ravel(), gn + gf)
        # spd 0 block against central differences of the restated gradient
        Hfd = np.zeros((12, 12))
        for j in range(12):
            for sgn in (1, -1):
                Z = X.copy(); Z.flat[j] += sgn * 1e-7
                Hfd[:, j] += sgn * (en.grad_cs(fn, Z) + en.grad_cs(ff, Z)) / 2e-7
        assert np.abs(H0[i] - Hfd).max() <= 1e-5 * np.abs(Hfd).max(), (i, np.abs(H0[i] - Hfd).max(), np.abs(Hfd).max())
        lam = np.linalg.eigvalsh(0.5 * (H1[i] + H1[i].T))
        assert lam.min() >= -1e-10 * np.abs(H1[i]).max()
        assert en.line_distance(X) < eps
    assert (fr_norm > 0) == (mu > 0)
    free = slice(3 * sc["n_lower"], None)   # (frozen rows of the gradient are zero)
    assert np.abs(g_c[free]).max() > 0
    assert np.abs(g_c[free] - g_ref[free]).max() <= 1e-12 * np.abs(g_ref[free]).max() * 10, np.abs(g_c[free] - g_ref[free]).max() / np.abs(g_ref[free]).max()
    assert abs(E_c - E_ref) <= 1e-9 * abs(E_ref), (E_c, E_ref)


# ------------------------------------------------------------------------------------------------ adjoint
def _tape(sc, ctx, T, x0):
    xs, sts = _rollout(ctx, sc, T, x0)
    return xs, sts


def test_adjoint_matches_rollout_differences():
    T = 6
    sc = en.bar_scene(gap=3e-4, mu="cloth_cloth")
    NV = len(sc["x"]); nl = sc["n_lower"]
    rng = np.random.default_rng(4)
    wgt = np.zeros((NV, 3)); wgt[nl:] = rng.normal(size=(NV - nl, 3)) * 1e-2
    mu0 = 0.4

    def make(mu):
        ctx = en.bar_context(sc)
        ctx.set_param("contact_ee", 1)
        ctx.set_param("mu_cloth_cloth", mu)
        ctx.set_param("cg_tol", 1e-13)
        return ctx

    def loss(x0, mu=mu0):
        ctx = make(mu)
        xs, sts = _tape(sc, ctx, T, x0)
        ctx.close()
        return float((wgt * xs[-1]).sum()), sts

    ctx = make(mu0)
    xs, sts = _tape(sc, ctx, T, sc["x"])
    assert all(c[0] == 0 and c[1] > 0 for _, c in sts) and all(st["unconverged"] == 0 for st, _ in sts)
    pb = torch.tensor(xs, device="cuda").contiguous()
    pg = torch.zeros_like(pb); pg[T - 1] = torch.tensor(wgt, device="cuda")
    rb = torch.zeros((T, 3), dtype=torch.float64, device="cuda"); ag = torch.zeros_like(rb)
    tz = torch.zeros(3 * NV, dtype=torch.float64, device="cuda")
    from thinshelllab_amd._lib import TslError
    for st_ in range(T - 1, 0, -1):
        ctx.adjoint_step(st_, T, pb, pg, rb, ag, tz, 1.0)
        # the friction-coefficient gradient of edge-edge slots is not implemented: the call fails instead of returning a number
        with pytest.raises(TslError, match="edge-edge"):
            ctx.friction_grad(pb[st_])
    g0 = pg[0].cpu().numpy()
    ctx.close()
    h = 1e-7
    dofs = [3 * v + a for v in (nl, nl + 5, NV - 1) for a in range(3)]
    for i in dofs:
        xp = sc["x"].copy(); xp.flat[i] += h
        xm = sc["x"].copy(); xm.flat[i] -= h
        (lp, sp), (lm, sm) = loss(xp), loss(xm)
        assert [c for _, c in sp] == [c for _, c in sts] == [c for _, c in sm]
        fd = (lp - lm) / (2 * h)
        assert abs(fd - g0.flat[i]) <= 1e-4 * np.abs(g0[nl:]).max(), (i, fd, g0.flat[i])


# ------------------------------------------------------------------------------------------------ solvers, determinism, groups
def test_direct_and_iterative_agree_and_runs_repeat():
    T = 10
    sc = en.bar_scene(gap=5e-4)
    tapes = {}
    for direct, rep in ((0, 0), (1, 0), (1, 1)):
        ctx = en.bar_context(sc)
        ctx.set_param("contact_ee", 1)
        ctx.set_param("direct", direct)
        xs, sts = _rollout(ctx, sc, T)
        assert all(st["unconverged"] == 0 for st, _ in sts) and max(c[1] for _, c in sts) > 0
        tapes[(direct, rep)] = (xs, [(st["nc"], st["newton_iters"], c) for st, c in sts])
        ctx.close()
    assert np.abs(tapes[(0, 0)][0] - tapes[(1, 0)][0]).max() < 1e-9
    assert np.array_equal(tapes[(1, 0)][0], tapes[(1, 1)][0]) and tapes[(1, 0)][1] == tapes[(1, 1)][1]


def test_group_member_matches_single_scene():
    from thinshelllab_amd import _lib
    from thinshelllab_amd._lib import StepStats, check
    from thinshelllab_amd.context import _ptr
    T = 6
    scs = [en.bar_scene(gap=5e-4), en.bar_scene(gap=7e-4, angle=np.pi / 2.5)]

    def ctxs():
        out = []
        for sc in scs:
            c = en.bar_context(sc)
            c.set_param("contact_ee", 1)
            c.set_param("direct", 1)
            out.append(c)
        return out
    single = []
    for sc, c in zip(scs, ctxs()):
        single.append(_rollout(c, sc, T))
        c.close()
    cs = ctxs()
    L = _lib.load()
    gh = C.c_void_p()
    check(L.tsl_group_create((C.c_void_p * 2)(*[c.h for c in cs]), 2, C.byref(gh)), "tsl_group_create")
    states = [_state(sc) for sc in scs]
    xs = [[st[0].cpu().numpy().copy()] for st in states]
    counts = [[], []]
    try:
        for _ in range(1, T):
            for c in cs:
                c.refresh_stream()
            arrs = [(C.c_void_p * 2)(*[_ptr(st[k]) for st in states]) for k in range(4)]
            stats = (StepStats * 2)()
            check(L.tsl_group_step(gh, *arrs, stats), "tsl_group_step")
            for i in range(2):
                xs[i].append(states[i][0].cpu().numpy().copy())
                counts[i].append(cs[i].contact_counts())
    finally:
        L.tsl_group_destroy(gh)
    for i in range(2):
        assert max(c[1] for c in counts[i]) > 0
        assert counts[i] == [c for _, c in single[i][1]]
        assert np.array_equal(np.array(xs[i]), single[i][0]), (i, np.abs(np.array(xs[i]) - single[i][0]).max())
